"""Multiprecision (mpmath, 50 digits) assembler and point locator for every mesh kind the library takes: (M, N) in {(1,1), (1,2), (2,2), (2,3),
(3,3)}, orders 1 and 2 -- the reference of tests/test_mp_ref_cpu.py and tests/test_gpu_geometry_robustness.py (a helper module, not a conftest).

Why it exists: every other checker of the suite is float64 (the C oracle, surface_ref.py, segment_ref.py), so where a kernel and its checker
differ nobody can say which is right, and where they agree they may share a loss.  Here the inputs are the float64 numbers exactly as the
kernels receive them (node coordinates, coefficients, the quadrature and reference-basis tables of the float64 checkers, every one converted
exactly: a float64 is a rational), all arithmetic runs in 50 digits, and a result is rounded once, by whoever compares it.

Written from the reference's formulas as surface_ref.py's docstring lists them, not from the HIP code:
  * per cell (geometry/simplex.h:184-195): J = [x1 - x0, ..., xM - x0] (N x M), J+ = (J^T J)^{-1} J^T (M x N; the inverse when N = M),
    measure = sqrt(det J^T J) / M!; kappa_2(J) = sqrt(lambda_max / lambda_min) of J^T J;
  * physical gradients g_i = J+^T dpsi_i; laplacian -(g_i . g_j), diffusion -(g_i . K g_j), advection psi_i (g_j . b), reaction c psi_i psi_j, dt 0;
    K_e[i][j] = |e| sum_q w_q form(q), coefficients constant or one value per quadrature node (row nq * cell + q);
  * an expression without an advection leaf: only the pairs dof_i >= dof_j are integrated, the lower triangle is mirrored (fem_assembler.h:94-117);
  * forcing b_i += |e| sum_q f_q psi_i(p_q) w_q; lumped mass = row sums; cell integrals int_e psi_h = |e| sum_q w_q psi_h(p_q).

Next to every assembled entry stands its SCALE  S_ij = sum_{cells e holding i and j} sum_{terms t} ||K_{e,t}||max  (force: S_i = sum_e max_h |f_{e,h}|):
the size of what was added up to make the entry, which is what a rounding error is relative to -- not the entry itself (entries cancel) and not
the matrix' largest entry (a floor that makes the check absolute).  S[0] is that sum; S[1] weights every cell's share by the growth the
reference's own float64 formulas show on stretched-then-rotated cells (growth_powers): kappa_2(J)^pj for the terms that hold a J+ (laplacian,
diffusion, advection) and kappa_2(J)^pm for those that hold the measure only (reaction, forcing, cell integrals) -- the determinant of a
stretched-then-rotated cell cancels, so the measure itself is only good to u kappa.  Segments: pj = pm = 0 (|J| is a square root of a sum of
squares); triangles in the plane and tetrahedra pj = pm = 1 (the adjugate inverse loses what the determinant loses); surface triangles pj = 2,
pm = 1 (the pseudo-inverse goes through J^T J, whose condition is kappa^2).  Measured on the float64 checkers over the whole case list
(tests/test_mp_ref_cpu.py: with these powers no ratio exceeds 7 u from kappa = 1 to 1.8e8; DESIGN.md section 5 has the table)."""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

import mpmath
import numpy as np
from mpmath import mp, mpf

import segment_ref as sg
from oracle import oracle as o

mp.dps = 50
U = 2.0 ** -53
ZERO, ONE = mpf(0), mpf(1)
LAPLACIAN, DIFFUSION, ADVECTION, REACTION, DT = o.LAPLACIAN, o.DIFFUSION, o.ADVECTION, o.REACTION, o.DT
HAS_JPLUS = (LAPLACIAN, DIFFUSION, ADVECTION)


def M_(x):
    """a float64 (or an exact Fraction) as an mpf, exactly"""
    if isinstance(x, Fraction):
        return mpf(x.numerator) / mpf(x.denominator)
    return mpf(float(x))


# ---- tables: the float64 checkers' own, converted exactly ------------------------------------------------------------------------------
_TABLES = {}


def tables(M, order):
    """-> qn (nq x M), qw (nq), psi (nb x nq), dpsi (nb x nq x M) as nested lists of mpf; float64 tables of the oracle (M = 2, 3) and of
    segment_ref (M = 1)"""
    if (M, order) not in _TABLES:
        if M == 1:
            qn, qw, psi, dpsi = sg.tables(order)
            qn, dpsi = qn.reshape(-1, 1), dpsi[:, :, None]
        else:
            o.build()
            qn, qw = o.quadrature(M, order)
            psi, dpsi = o.basis_tables(M, order)
        cv = lambda a: [cv(x) for x in a] if getattr(a, "ndim", 0) > 0 else mpf(float(a))
        _TABLES[(M, order)] = (cv(qn), cv(qw), cv(psi), cv(dpsi))
    return _TABLES[(M, order)]


def exact_tables(M):
    """the order-1 rules with their constants in 50 digits instead of the 15 printed ones (integrator_tables.h): 2-point Gauss on [0, 1]; the
    3-point rule (1/6, 1/6), (2/3, 1/6), (1/6, 2/3) on the triangle; the 4-point rule with a = (5 - sqrt 5) / 20 on the tetrahedron -- exact for
    the quadratic integrands of the P1 mass matrix, which is what the closed-form tests need.  Same node order as tables(M, 1)."""
    if M == 1:
        r = 1 / (2 * mpmath.sqrt(3))
        qn, qw = [[mpf(1) / 2 - r], [mpf(1) / 2 + r]], [mpf(1) / 2] * 2
    elif M == 2:
        a, b = mpf(1) / 6, mpf(2) / 3
        qn, qw = [[a, a], [b, a], [a, b]], [mpf(1) / 3] * 3
    else:
        a = (5 - mpmath.sqrt(5)) / 20
        b = 1 - 3 * a
        qn, qw = [[b, a, a], [a, a, a], [a, a, b], [a, b, a]], [mpf(1) / 4] * 4
    psi = [[ONE - sum(q) for q in qn]] + [[q[k] for q in qn] for k in range(M)]
    dpsi = [[[-ONE] * M for _ in qn]] + [[[ONE if d == k else ZERO for d in range(M)] for _ in qn] for k in range(M)]
    return qn, qw, psi, dpsi


def reference_nodes(M, order):
    """reference DOF nodes as barycentric tuples of Fractions (lambda_0 .. lambda_M): ReferenceElement<M, R>"""
    if M == 1:
        ref = [[0.0], [1.0]] + ([[0.5]] if order == 2 else [])
    else:
        o.build()
        ref = o.reference_nodes(M, order).tolist()
    out = []
    for r in ref:
        f = [Fraction(x) for x in r]
        out.append(tuple([1 - sum(f)] + f))
    return out


def basis_at(M, order, lam):
    """Lagrange basis of the reference element at barycentric coordinates lam (M + 1 mpf), in the order of reference_nodes(): P1 lambda_a; P2
    lambda_a (2 lambda_a - 1) at a vertex, 4 lambda_a lambda_b at the midpoint of (a, b)"""
    out = []
    for node in reference_nodes(M, order):
        nz = [a for a in range(M + 1) if node[a] != 0]
        if len(nz) == 1:
            a = nz[0]
            out.append(lam[a] if order == 1 else lam[a] * (2 * lam[a] - 1))
        else:
            assert order == 2 and len(nz) == 2 and node[nz[0]] == Fraction(1, 2)
            out.append(4 * lam[nz[0]] * lam[nz[1]])
    return out


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def _det(A):
    n = len(A)
    if n == 1:
        return A[0][0]
    if n == 2:
        return A[0][0] * A[1][1] - A[0][1] * A[1][0]
    return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
            + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))


def _inv(A):
    n, d = len(A), _det(A)
    if n == 1:
        return [[ONE / d]]
    if n == 2:
        return [[A[1][1] / d, -A[0][1] / d], [-A[1][0] / d, A[0][0] / d]]
    C = [[ZERO] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            m = [[A[r][c] for c in range(3) if c != j] for r in range(3) if r != i]
            C[j][i] = (-1) ** (i + j) * _det(m) / d
    return C


class Cell:
    """x (M+1 vertices x N), J (N x M), Jp = J+ (M x N), measure, kappa = kappa_2(J), jp_inf = the largest absolute row sum of the (M+1) x N
    matrix of barycentric gradients (the rows of J+ and minus their sum)"""

    def __init__(self, x):
        self.x = x
        M, N = len(x) - 1, len(x[0])
        self.M, self.N = M, N
        self.J = [[x[k + 1][d] - x[0][d] for k in range(M)] for d in range(N)]
        G = [[sum(self.J[d][a] * self.J[d][b] for d in range(N)) for b in range(M)] for a in range(M)]
        Gi = _inv(G)
        self.Jp = [[sum(Gi[a][b] * self.J[d][b] for b in range(M)) for d in range(N)] for a in range(M)]
        self.measure = mpmath.sqrt(_det(G)) / math.factorial(M)
        if M == 1:
            self.kappa = 1.0
        elif M == 2:
            h = (G[0][0] + G[1][1]) / 2
            lmax = h + mpmath.sqrt(h * h - _det(G))
            self.kappa = float(mpmath.sqrt(lmax * lmax / _det(G)))
        else:
            ev = mp.eigsy(mp.matrix(G), eigvals_only=True)
            self.kappa = float(mpmath.sqrt(max(ev) / min(ev)))
        rows = self.Jp + [[-sum(self.Jp[a][d] for a in range(M)) for d in range(N)]]
        self.jp_inf = float(max(sum(abs(v) for v in r) for r in rows))
        self.xmax = float(max(abs(v) for p in x for v in p))

    def barycentric(self, p):
        """(lambda_0 .. lambda_M) of p (N mpf); for N > M of p's orthogonal projection onto the cell's plane / line"""
        d = [p[k] - self.x[0][k] for k in range(self.N)]
        xi = [sum(self.Jp[a][k] * d[k] for k in range(self.N)) for a in range(self.M)]
        return [ONE - sum(xi)] + xi

    def distance(self, p):
        """distance of p to the cell's affine hull"""
        lam = self.barycentric(p)
        r = [p[k] - sum(lam[a] * self.x[a][k] for a in range(self.M + 1)) for k in range(self.N)]
        return mpmath.sqrt(sum(v * v for v in r))

    def length(self):
        return mpmath.sqrt(sum(self.J[d][0] ** 2 for d in range(self.N)))


def growth_powers(M, N):
    """(pj, pm): powers of kappa_2(J) that weight the terms with a J+ and the terms with the measure only"""
    if M == 1:
        return 0, 0
    return (2, 1) if (M, N) == (2, 3) else (1, 1)


class Space:
    """one mesh at one order: cells in 50 digits, DOF table, CSR pattern (every pair of DOFs that share a cell, sorted), and a cache of the
    element matrices of the terms asked for so far"""

    def __init__(self, nodes, cells, dofs, n_dofs, order, exact=False):
        """exact: order 1 with the quadrature constants in 50 digits (exact_tables) instead of the checkers' float64 tables"""
        nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
        self.nodes, self.cells_idx, self.dofs, self.n_dofs, self.order = nodes, np.asarray(cells), np.asarray(dofs), int(n_dofs), order
        self.M, self.N = self.cells_idx.shape[1] - 1, nodes.shape[1]
        mpn = [[mpf(float(v)) for v in p] for p in nodes]
        self.cells = [Cell([mpn[v] for v in c]) for c in self.cells_idx]
        assert not exact or order == 1
        self.qn, self.qw, self.psi, self.dpsi = exact_tables(self.M) if exact else tables(self.M, order)
        self.nb, self.nq = len(self.psi), len(self.qw)
        assert self.dofs.shape == (len(self.cells), self.nb)
        pairs = set()
        for row in self.dofs.tolist():
            pairs.update(itertools.product(row, row))
        pairs = sorted(pairs)
        self.pos = {ij: k for k, ij in enumerate(pairs)}
        self.rows = np.array([ij[0] for ij in pairs], np.int64)
        self.colidx = np.array([ij[1] for ij in pairs], np.int32)
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=self.n_dofs))]).astype(np.int32)
        self._grad, self._term = None, {}

    # -- per-cell ingredients
    def kappa(self):
        return np.array([c.kappa for c in self.cells])

    def measures(self):
        return [c.measure for c in self.cells]

    def quadrature_nodes(self):
        """(n_cells nq) x N mpf: x0 + J p_q, rows nq cell + q"""
        out = []
        for c in self.cells:
            for q in range(self.nq):
                out.append([c.x[0][d] + sum(c.J[d][k] * self.qn[q][k] for k in range(self.M)) for d in range(self.N)])
        return out

    def measure_weights(self):
        """kappa_2(J)^pm per cell: what the float64 measure of the cell is good to, in units of u"""
        return self.kappa() ** growth_powers(self.M, self.N)[1]

    def cell_integrals(self):
        """-> (n_cells x nb) mpf: |e| sum_q w_q psi_h(p_q)"""
        s = [sum(self.psi[h][q] * self.qw[q] for q in range(self.nq)) for h in range(self.nb)]
        return [[c.measure * v for v in s] for c in self.cells]

    def gradients(self):
        if self._grad is None:
            self._grad = [[[[sum(c.Jp[k][r] * self.dpsi[i][q][k] for k in range(self.M)) for r in range(self.N)] for q in range(self.nq)]
                           for i in range(self.nb)] for c in self.cells]
        return self._grad

    def _coef(self, cst, data, e, shape):
        """coefficient of cell e at every quadrature node: nq values of the given shape (flat lists)"""
        n = int(np.prod(shape)) if shape else 1
        if data is None:
            v = [mpf(float(t)) for t in np.asarray(cst, float).reshape(-1)[:n]]
            return [v] * self.nq
        d = np.asarray(data, float).reshape(len(self.cells) * self.nq, n)
        return [[mpf(float(t)) for t in d[e * self.nq + q]] for q in range(self.nq)]

    def term_matrices(self, kind, cst, data):
        """element matrices of ONE leaf with coefficient 1: list over cells of nb x nb mpf"""
        key = (kind, None if cst is None else np.asarray(cst, float).tobytes(), None if data is None else np.asarray(data, float).tobytes())
        if key in self._term:
            return self._term[key]
        nb, nq, N, w, psi = self.nb, self.nq, self.N, self.qw, self.psi
        out = []
        g_all = self.gradients() if kind in HAS_JPLUS else None
        for e, c in enumerate(self.cells):
            K = [[ZERO] * nb for _ in range(nb)]
            if kind == DT:
                out.append(K)
                continue
            g = g_all[e] if g_all is not None else None
            if kind == LAPLACIAN:
                for i in range(nb):
                    for j in range(nb):
                        K[i][j] = -sum(w[q] * sum(g[i][q][r] * g[j][q][r] for r in range(N)) for q in range(nq)) * c.measure
            elif kind == DIFFUSION:
                Kq = self._coef(cst, data, e, (N, N))
                Kg = [[[sum(Kq[q][r * N + s] * g[j][q][s] for s in range(N)) for r in range(N)] for q in range(nq)] for j in range(nb)]
                for i in range(nb):
                    for j in range(nb):
                        K[i][j] = -sum(w[q] * sum(g[i][q][r] * Kg[j][q][r] for r in range(N)) for q in range(nq)) * c.measure
            elif kind == ADVECTION:
                bq = self._coef(cst, data, e, (N,))
                gb = [[sum(g[j][q][r] * bq[q][r] for r in range(N)) for q in range(nq)] for j in range(nb)]
                for i in range(nb):
                    for j in range(nb):
                        K[i][j] = sum(w[q] * psi[i][q] * gb[j][q] for q in range(nq)) * c.measure
            elif kind == REACTION:
                cq = self._coef(cst, data, e, ())
                for i in range(nb):
                    for j in range(nb):
                        K[i][j] = sum(w[q] * cq[q][0] * psi[i][q] * psi[j][q] for q in range(nq)) * c.measure
            else:
                raise ValueError(kind)
            out.append(K)
        self._term[key] = out
        return out

    # -- assembled objects
    def assemble(self, op):
        """op: an Operator of oracle.py / capi.py (terms (kind, coef, cst, data)) -> Assembled in this space's pattern"""
        terms = [(k, mpf(float(cf)), self.term_matrices(k, cst, data)) for (k, cf, cst, data) in op.terms]
        mirrored = not any(k == ADVECTION for (k, _, _, _) in op.terms)
        nnz, nb = len(self.pos), self.nb
        vals = [ZERO] * nnz
        S = np.zeros((2, nnz))
        pj, pm = growth_powers(self.M, self.N)
        for e, c in enumerate(self.cells):
            L = [[sum(cf * Kt[e][i][j] for (_, cf, Kt) in terms) for j in range(nb)] for i in range(nb)]
            s = np.zeros(2)
            for (k, cf, Kt) in terms:
                mx = float(abs(cf) * max(abs(v) for r in Kt[e] for v in r))
                s += mx * np.array([1.0, c.kappa ** (pj if k in HAS_JPLUS else pm)])
            d = self.dofs[e].tolist()
            for i in range(nb):
                for j in range(nb):
                    k = self.pos[(d[i], d[j])]
                    S[:, k] += s
                    if not mirrored:
                        vals[k] += L[i][j]
                    elif d[i] >= d[j]:
                        vals[k] += L[i][j]
                        if d[i] != d[j]:
                            vals[self.pos[(d[j], d[i])]] += L[i][j]
        return Assembled(vals, S)

    def forcing(self, f_q):
        f = np.asarray(f_q, float).reshape(len(self.cells), self.nq)
        vals, S = [ZERO] * self.n_dofs, np.zeros((2, self.n_dofs))
        pm = growth_powers(self.M, self.N)[1]
        for e, c in enumerate(self.cells):
            loc = [c.measure * sum(mpf(float(f[e, q])) * self.psi[i][q] * self.qw[q] for q in range(self.nq)) for i in range(self.nb)]
            mx = float(max(abs(v) for v in loc))
            for i, dof in enumerate(self.dofs[e].tolist()):
                vals[dof] += loc[i]
                S[:, dof] += mx * np.array([1.0, c.kappa ** pm])
        return Assembled(vals, S)

    def lumped(self, A):
        """row sums of an Assembled matrix (lump(mass())): the scale of a row is the sum of its entries' scales"""
        vals, S = [ZERO] * self.n_dofs, np.zeros((2, self.n_dofs))
        for k, r in enumerate(self.rows.tolist()):
            vals[r] += A.vals[k]
            S[:, r] += A.S[:, k]
        return Assembled(vals, S)

    # -- point location
    def rho(self, e, p):
        """what the float64 rounding of a location and of the vertices is worth in barycentric units of cell e: 4 u max(|p|, |x_i|) ||J+||_inf"""
        c = self.cells[e]
        return 4.0 * U * max(float(np.abs(np.asarray(p, float)).max()), c.xmax) * c.jp_inf

    def candidates(self, p, tol=1e-12, k=1.0, prefilter=1e-4):
        """C(tau): ids of the cells whose barycentric coordinates of p are all >= -tau (segments in the plane: and whose line is within
        tau * length of p), with tau = tol + k rho(cell, p) per cell.  float64 is only used to discard cells that miss by more than `prefilter`."""
        p64 = np.asarray(p, float).reshape(-1)
        if not hasattr(self, "_pre"):
            x0 = self.nodes[self.cells_idx[:, 0]]
            Jm = np.stack([self.nodes[self.cells_idx[:, k + 1]] - x0 for k in range(self.M)], axis=2)   # (m, N, M)
            self._pre = (x0, np.linalg.pinv(Jm))
        x0, Jp = self._pre
        xi = np.einsum("mkd,md->mk", Jp, p64[None, :] - x0)
        lam = np.concatenate([1.0 - xi.sum(axis=1, keepdims=True), xi], axis=1)
        near = np.nonzero(lam.min(axis=1) >= -prefilter)[0]
        pm = [mpf(float(v)) for v in p64]
        out = []
        for e in near.tolist():
            c = self.cells[e]
            tau = tol + k * self.rho(e, p64)
            assert tau < 0.1 * prefilter, "rho too large for the float64 prefilter"
            if min(c.barycentric(pm)) >= -tau and (self.N == self.M or c.distance(pm) <= tau * c.length()):
                out.append(e)
        return out

    def psi_row(self, e, p):
        """-> (DOF ids of cell e, basis values at p's barycentric coordinates in cell e, the coordinates)"""
        lam = self.cells[e].barycentric([mpf(float(v)) for v in np.asarray(p, float).reshape(-1)])
        return self.dofs[e].tolist(), basis_at(self.M, self.order, lam), lam


class Assembled:
    """vals: mpf per entry (pattern order / per DOF); S[0]: the plain scale, S[1]: every cell's share weighted by its growth (growth_powers)"""

    def __init__(self, vals, S):
        self.vals, self.S = vals, S

    def rounded(self):
        return np.array([float(v) for v in self.vals])

    def ratio(self, got, p=1):
        """worst |got - self| / (u S[p]) over the entries, computed in 50 digits; an entry of scale 0 must be matched exactly"""
        got = np.asarray(got, float).reshape(-1)
        assert got.size == len(self.vals)
        worst = 0.0
        for k, v in enumerate(self.vals):
            d = float(abs(mpf(float(got[k])) - v))
            s = self.S[p, k]
            worst = max(worst, (0.0 if d == 0.0 else math.inf) if s == 0.0 else d / (U * s))
        return worst


def ratio_plain(got, ref, scale):
    """worst |got - ref| / (u scale) for flat sequences: got float64, ref mpf, scale float64 (per entry)"""
    got = np.asarray(got, float).reshape(-1)
    worst = 0.0
    for g, r, s in zip(got.tolist(), ref, np.broadcast_to(np.asarray(scale, float).reshape(-1), got.shape).tolist()):
        worst = max(worst, float(abs(mpf(g) - r)) / (U * s))
    return worst


# ---- the case list shared by tests/test_mp_ref_cpu.py and tests/test_gpu_geometry_robustness.py ----------------------------------------
# (kind, mesh, scale, shifted, stretch, rotated): nodes -> scale * R (diag(stretch, 1, ..) x) + shift, shift = 1e6 * scale in every coordinate
# when `shifted` ("metres" is the street network in projected metres: scale 100, shift (5e5, 4.5e6)).  Every stretched case is rotated after the
# stretch -- an axis-aligned stretch loses nothing; (2,3) and (1,2) are always rotated.  Every value of every axis appears, and the worst
# corners (largest stretch with the largest shift and both extreme scales).
CASES = [
    # (1,1): intervals (the stretch of the one axis is a scale)
    ("11", "interval", 1.0, False, 1.0, False), ("11", "interval", 1e-6, True, 1.0, False), ("11", "interval", 1e6, True, 1.0, False),
    ("11", "interval", 1.0, True, 1e3, False), ("11", "interval", 1.0, False, 1e6, False), ("11", "interval", 1e-6, True, 1e6, False),
    # (1,2): street networks, always oblique
    ("12", "streets", 1.0, False, 1.0, True), ("12", "streets", 1.0, True, 1.0, True), ("12", "streets", 1e-6, True, 1.0, True),
    ("12", "streets", 1e6, True, 1.0, True), ("12", "streets", 1.0, True, 1e3, True), ("12", "streets", 1.0, False, 1e6, True),
    ("12", "streets", 1e6, False, 1e3, True), ("12", "streets", 1e-6, True, 1e6, True), ("12", "streets", 100.0, "metres", 1.0, True),
    # (2,2): triangles
    ("22", "square", 1.0, False, 1.0, False), ("22", "square", 1.0, True, 1.0, False), ("22", "square", 1e-6, True, 1.0, True),
    ("22", "square", 1e6, True, 1.0, True), ("22", "square", 1.0, False, 1e3, True), ("22", "square", 1.0, True, 1e3, True),
    ("22", "square", 1.0, False, 1e6, True), ("22", "square", 1e-6, True, 1e6, True), ("22", "square", 1e6, True, 1e3, True),
    # (2,3): surfaces, always rotated
    ("23", "sphere", 1.0, False, 1.0, True), ("23", "sphere", 1e-6, True, 1.0, True), ("23", "sphere", 1e6, True, 1.0, True),
    ("23", "sphere", 1.0, False, 30.0, True), ("23", "sphere", 1.0, True, 1e3, True), ("23", "height", 1.0, True, 1.0, True),
    ("23", "height", 1.0, False, 30.0, True), ("23", "height", 1e6, False, 1e3, True), ("23", "height", 1e-6, True, 1e3, True),
    # (3,3): tetrahedra; "slivers" = the cube with a cap, a needle and a sliver (volume / h^3 down to 1e-9) glued on
    ("33", "cube", 1.0, False, 1.0, False), ("33", "cube", 1e-6, True, 1.0, True), ("33", "cube", 1e6, True, 1.0, True),
    ("33", "cube", 1.0, False, 30.0, True), ("33", "cube", 1.0, True, 1e3, True), ("33", "cube", 1e6, True, 1e3, True),
    ("33", "cube", 1e-6, False, 1e3, True), ("33", "slivers", 1.0, False, 1.0, False), ("33", "slivers", 1.0, True, 1.0, True),
]
ORDERS = (1, 2)


def case_id(case):
    k, mesh, scale, shifted, stretch, rot = case
    return f"{k}-{mesh}-s{scale:g}-{'metres' if shifted == 'metres' else ('shift' if shifted else 'noshift')}-x{stretch:g}-{'rot' if rot else 'axis'}"


def _meshgen():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen

    return meshgen


def sliver_cube(meshgen):
    """unit_cube(2) without jitter, plus three degenerate tetrahedra: a CAP (apex 1e-8 above the centroid of a boundary face: volume / h^3 ~ 1e-9),
    a NEEDLE (apex 8e3 above another boundary face: ~ 1e-9 of its longest edge cubed) and a SLIVER (two edges of length 0.5 crossing at a
    distance of 3e-9, one of them a boundary edge of the cube)"""
    nodes, cells, bnd = meshgen.unit_cube(2, jitter=0.0, permute=False)
    nodes, cells, bnd = nodes.copy(), cells.astype(np.int64), bnd.copy()
    faces = {}
    for c in cells:
        for f in itertools.combinations(sorted(c.tolist()), 3):
            faces[f] = faces.get(f, 0) + 1
    bfaces = sorted(f for f, n in faces.items() if n == 1)
    top = [f for f in bfaces if np.all(nodes[list(f), 2] == 1.0)][0]
    side = [f for f in bfaces if np.all(nodes[list(f), 0] == 1.0)][0]
    new_nodes, new_cells = [], []
    n = nodes.shape[0]
    new_nodes.append(nodes[list(top)].mean(axis=0) + np.array([0.0, 0.0, 1e-8]))
    new_cells.append(list(top) + [n])
    new_nodes.append(nodes[list(side)].mean(axis=0) + np.array([8e3, 0.0, 0.0]))
    new_cells.append(list(side) + [n + 1])
    a, b = [f for f in bfaces if np.all(nodes[list(f), 1] == 0.0)][0][:2]   # an edge of the face y = 0
    mid, d = 0.5 * (nodes[a] + nodes[b]), nodes[b] - nodes[a]
    t = np.cross(d, [0.0, 1.0, 0.0])
    t *= 0.25 / np.linalg.norm(t)
    new_nodes += [mid + np.array([0.0, -3e-9, 0.0]) + t, mid + np.array([0.0, -3e-9, 0.0]) - t]
    new_cells.append([a, b, n + 2, n + 3])
    nodes = np.vstack([nodes] + [x[None] for x in new_nodes])
    cells = np.vstack([cells, np.array(new_cells, np.int64)])
    bnd = np.concatenate([bnd, np.ones(4, np.uint8)])
    return np.ascontiguousarray(nodes), np.ascontiguousarray(cells.astype(np.int32)), bnd


def rotation_of(N):
    if N == 1:
        return np.eye(1)
    if N == 2:
        c, s = math.cos(0.5), math.sin(0.5)
        return np.array([[c, -s], [s, c]])
    return _meshgen().rotation(4)


def build_mesh(case):
    """-> nodes (n, N) float64 C-order, cells int32, boundary uint8 of a case of CASES"""
    k, mesh, scale, shifted, stretch, rot = case
    mg = _meshgen()
    base = {"interval": lambda: mg.interval(24, jitter=0.3, permute=True), "streets": lambda: mg.street_grid(3, 3, k=3),
            "square": lambda: mg.unit_square(4), "sphere": lambda: mg.unit_sphere_surface(1, permute=True),
            "height": lambda: mg.height_field_surface(4, seed=7, reorient=True), "cube": lambda: mg.unit_cube(2),
            "slivers": lambda: sliver_cube(mg)}[mesh]()
    nodes, cells, bnd = base
    N = nodes.shape[1]
    shift = np.array([5e5, 4.5e6]) if shifted == "metres" else (1e6 * scale if shifted else 0.0) * np.ones(N)
    return mg.transform(nodes, scale=scale, shift=shift, stretch=stretch, rotation=rotation_of(N) if rot else None), cells, bnd


def enumerate_dofs(nodes, cells, bnd, order):
    """-> (dofs, boundary DOFs, n_dofs) by the float64 checkers' numbering (segment_ref for segments, the oracle otherwise)"""
    if cells.shape[1] == 2:
        return sg.dofs(cells, nodes.shape[0], bnd, order)
    o.build()
    d, b, nd, _ = o.enumerate_dofs(o.Mesh(np.ascontiguousarray(nodes), np.ascontiguousarray(cells, np.int32), np.ascontiguousarray(bnd, np.uint8)), order)
    return d, b, nd


def operators(mod, N, rows, seed=5):
    """the expressions of the robustness tests for a module with the operator algebra (oracle.py or capi.py): -laplacian, mass,
    diffusion(K) + advection(b) + reaction(c) with the NON-symmetric K of tests/test_gpu_surface.py::_ops3, the same without advection (the
    reference's mirrored form), and one expression of per-quadrature-node K, b, c fields"""
    K = np.array([[2.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 1.5]])
    Kn = (K + np.array([[0.0, 0.4, 0.0], [-0.2, 0.0, 0.3], [0.1, -0.3, 0.0]]))[:N, :N]
    b = np.array([0.7, -0.2, 0.4])[:N]
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((rows, N, N)) * 0.3
    Kq = (np.einsum("rij,rkj->rik", A, A) + np.eye(N)[None]).reshape(rows, N * N)
    bq = rng.standard_normal((rows, N))
    cq = rng.uniform(0.5, 2.0, rows)
    return {"neg_laplacian": -mod.laplacian(), "mass": mod.reaction(1.0),
            "nonsym_adv": mod.diffusion(Kn) + mod.advection(b) + mod.reaction(0.5), "nonsym_mirrored": mod.diffusion(Kn) + mod.reaction(0.5),
            "fields": mod.diffusion_field(Kq) + mod.advection_field(bq) + mod.reaction_field(cq)}


def forcing_samples(rows, seed=11):
    return np.random.default_rng(seed).standard_normal(rows)


_SPACES = {}


def space_of(case, order):
    """the case's mesh, numbering and multiprecision space, built once per process"""
    key = (case, order)
    if key not in _SPACES:
        nodes, cells, bnd = build_mesh(case)
        dofs, bdofs, nd = enumerate_dofs(nodes, cells, bnd, order)
        _SPACES[key] = (nodes, cells, bnd, dofs, bdofs, nd, Space(nodes, cells, dofs, nd, order))
    return _SPACES[key]


# ---- locations off the unit box -----------------------------------------------------------------------------------------------------------
def is_location_case(case):
    """point location is tested on the transformed meshes with stretch <= 1e3; not on surfaces (refused by design) and not on the hand-made
    slivers (kappa ~ 1e8: a float64 location is worth more than a whole barycentric unit there)"""
    k, mesh, scale, shifted, stretch, rot = case
    return k != "23" and mesh != "slivers" and stretch <= 1e3


def location_points(sp, seed=3, per_kind=120):
    """locations built in float64 as convex combinations of cell vertices -> (inside (n, N), home cell of each, outside (k, N)):
    every mesh node; points on shared edges (2-D), faces and edges (3-D), segments and their junctions (1-D); random interior points; and points
    OUTSIDE by 1e-3 of the local cell size: across a boundary facet (barycentric coordinate -1e-3 of the opposite vertex), beyond the ends of an
    interval, off a network segment's line by 1e-3 of its length"""
    rng = np.random.default_rng(seed)
    X, cells, M, N = sp.nodes, sp.cells_idx, sp.M, sp.N
    m = len(cells)
    pts, home = [], []
    first = {}
    for e, c in enumerate(cells.tolist()):
        for v in c:
            first.setdefault(v, e)
    for v in range(len(X)):   # every node
        pts.append(X[v]), home.append(first[v])
    sub = {}   # lower-dimensional faces: vertex tuple -> cells holding it
    for e, c in enumerate(cells.tolist()):
        for d in range(2, M + 1):
            for f in itertools.combinations(sorted(c), d):
                sub.setdefault(f, []).append(e)
    shared = [f for f in sorted(sub) if len(sub[f]) > 1] if M > 1 else []
    for f in [shared[i] for i in rng.permutation(len(shared))[:per_kind]]:
        for _ in range(2):
            w = rng.dirichlet(np.ones(len(f)))
            pts.append(w @ X[list(f)]), home.append(sub[f][0])
    for e in rng.integers(0, m, per_kind):   # interior (for segments: on the segment)
        w = rng.dirichlet(np.ones(M + 1))
        pts.append(w @ X[cells[e]]), home.append(int(e))
    out = []
    if M == 1 and N == 1:
        lo, hi = X[:, 0].min(), X[:, 0].max()
        h = (hi - lo) / m
        out = [[lo - 1e-3 * h], [hi + 1e-3 * h]]
    elif M == 1:
        for e in rng.integers(0, m, per_kind // 2):
            a, b = X[cells[e, 0]], X[cells[e, 1]]
            t = rng.uniform(0.3, 0.7)
            d = b - a
            out.append(a + t * d + 1e-3 * np.array([-d[1], d[0]]) * rng.choice([-1.0, 1.0]))
    else:
        bfac = [f for f in sorted(sub) if len(f) == M and len(sub[f]) == 1]
        for f in [bfac[i] for i in rng.permutation(len(bfac))[:per_kind // 2]]:
            e = sub[f][0]
            opp = [v for v in cells[e].tolist() if v not in f][0]
            w = rng.dirichlet(np.ones(M)) * 1.001
            out.append(w @ X[list(f)] - 1e-3 * X[opp])
    return np.array(pts, float).reshape(-1, N), np.array(home, np.int64), np.array(out, float).reshape(-1, N)
