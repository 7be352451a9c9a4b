"""A float64 numpy restatement of fdapde_project (nearest cell, closest point, distance, barycentric coordinates), vectorised over
(point, cell) pairs, with a brute force over all cells; mpmath helpers that judge a claimed closest point from first principles; and
constructed points with known answers for every Voronoi region of one cell.  No GPU.

Closest point per cell: a segment clamps its parameter; a triangle (in R^2 or R^3) tests the Voronoi regions of its vertices, edges and face
through dot products (Ericson, Real-Time Collision Detection, 5.1.5); a tetrahedron returns the point itself where all barycentric coordinates
are >= 0 and the best of its four faces' closest points otherwise.

The first-principles characterisation (closest_point_defects): q is THE closest point of the convex cell K = conv(x_0 .. x_M) to p iff q is in K
and (p - q).(x - q) <= 0 for every x in K, which by linearity is (p - q).(x_v - q) <= 0 for every vertex.  If q is within eps of the true closest
point, the barycentric coordinates are off by at most eps / (smallest height of the cell), the distance of q to the cell's plane or line by eps, and
(p - q).(x_v - q) by eps (|p - q| + |x_v - q|) to first order: these are the scales the defects are reported in, so that each is comparable to a
LENGTH tolerance."""
from __future__ import annotations

import itertools

import numpy as np
from mpmath import mp, mpf

DPS = 40   # (set around each evaluation: the global precision belongs to whoever imported mpmath first, tests/mp_ref.py among them)


# ---- float64, vectorised: p (n, N), vertices (n, N) each -> lam (n, M + 1), q (n, N), d2 (n,) ------------------------------------------------
def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def closest_segment(p, a, b):
    ab = b - a
    d1, d3 = _dot(ab, p - a), _dot(ab, p - b)
    lo, hi = d1 <= 0.0, ~(d1 <= 0.0) & (d3 >= 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip(d1 / (d1 - d3), 0.0, 1.0)
    t = np.where(lo, 0.0, np.where(hi, 1.0, t))
    q = a + t[..., None] * ab
    q = np.where(lo[..., None], a, np.where(hi[..., None], b, q))
    if p.shape[-1] == 1:
        q = np.where((~lo & ~hi)[..., None], p, q)
    lam = np.stack([1.0 - t, t], axis=-1)
    return lam, q, _dot(p - q, p - q)


def closest_triangle(p, a, b, c):
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    ra = (d1 <= 0) & (d2 <= 0)
    rb = ~ra & (d3 >= 0) & (d4 <= d3)
    rc = ~ra & ~rb & (d6 >= 0) & (d5 <= d6)
    done = ra | rb | rc
    rab = ~done & (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    done = done | rab
    rac = ~done & (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    done = done | rac
    rbc = ~done & (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
    face = ~(done | rbc)
    with np.errstate(divide="ignore", invalid="ignore"):
        vab = np.clip(d1 / (d1 - d3), 0, 1)
        wac = np.clip(d2 / (d2 - d6), 0, 1)
        wbc = np.clip((d4 - d3) / ((d4 - d3) + (d5 - d6)), 0, 1)
        den = 1.0 / (va + vb + vc)
        vf, wf = np.clip(vb * den, 0, 1), np.clip(vc * den, 0, 1)
    z, o = np.zeros_like(d1), np.ones_like(d1)
    lam = np.zeros(d1.shape + (3,))
    q = np.zeros(np.broadcast_shapes(p.shape, a.shape))
    for mask, l, qq in [(ra, (o, z, z), a), (rb, (z, o, z), b), (rc, (z, z, o), c),
                        (rab, (1 - vab, vab, z), a + vab[..., None] * ab), (rac, (1 - wac, z, wac), a + wac[..., None] * ac),
                        (rbc, (z, 1 - wbc, wbc), b + wbc[..., None] * (c - b)),
                        (face, (np.maximum(1 - vf - wf, 0), vf, wf), (p + 0 * a) if p.shape[-1] == 2 else a + vf[..., None] * ab + wf[..., None] * ac)]:
        lam = np.where(mask[..., None], np.stack(np.broadcast_arrays(*l), axis=-1), lam)
        q = np.where(mask[..., None], qq, q)
    return lam, q, _dot(p - q, p - q)


def closest_tetrahedron(p, x0, x1, x2, x3):
    rhs = p - x0
    J = np.broadcast_to(np.stack([x1 - x0, x2 - x0, x3 - x0], axis=-1), rhs.shape + (3,))
    xi = np.linalg.solve(J, rhs[..., None])[..., 0]
    l0 = 1.0 - xi.sum(axis=-1)
    inside = (l0 >= 0) & (xi >= 0).all(axis=-1)
    best = None
    for k, (f, cols) in enumerate([((x1, x2, x3), (1, 2, 3)), ((x0, x2, x3), (0, 2, 3)), ((x0, x1, x3), (0, 1, 3)), ((x0, x1, x2), (0, 1, 2))]):
        fl, fq, fd = closest_triangle(p, *f)
        lam = np.zeros(fd.shape + (4,))
        lam[..., cols] = fl
        if best is None:
            best = [lam, fq, fd]
        else:
            take = fd < best[2]
            best = [np.where(take[..., None], lam, best[0]), np.where(take[..., None], fq, best[1]), np.where(take, fd, best[2])]
    lam_in = np.minimum(np.concatenate([l0[..., None], xi], axis=-1), 1.0)
    lam = np.where(inside[..., None], lam_in, best[0])
    q = np.where(inside[..., None], p + 0 * x0, best[1])
    return lam, q, np.where(inside, 0.0, best[2])


def closest_on_cells(nodes, cells, pts):
    """every point against every cell: lam (n, m, M + 1), q (n, m, N), d2 (n, m)"""
    nodes = np.asarray(nodes, dtype=float).reshape(len(nodes), -1)
    P = np.asarray(pts, dtype=float).reshape(len(pts), -1)[:, None, :]
    V = [nodes[cells[:, k]][None, :, :] for k in range(cells.shape[1])]
    fn = {2: closest_segment, 3: closest_triangle, 4: closest_tetrahedron}[cells.shape[1]]
    return fn(P, *V)


def brute_force(nodes, cells, pts, chunk=256):
    """the nearest cell of every point over ALL cells (lowest cell id on equal computed squared distances) -> cell (n,), lam, q, dist"""
    pts = np.asarray(pts, dtype=float).reshape(len(pts), -1)
    out = [[], [], [], []]
    for s in range(0, len(pts), chunk):
        lam, q, d2 = closest_on_cells(nodes, cells, pts[s:s + chunk])
        k = np.argmin(d2, axis=1)   # (the first minimum: the lowest id)
        r = np.arange(len(k))
        for o_, v in zip(out, (k, lam[r, k], np.broadcast_to(q, d2.shape + (q.shape[-1],))[r, k], np.sqrt(d2[r, k]))):
            o_.append(v)
    return tuple(np.concatenate(v) for v in out)


# ---- mpmath: is q the closest point of the cell to p? --------------------------------------------------------------------------------------
def _mv(x):
    return [mpf(float(v)) for v in np.asarray(x, dtype=float).reshape(-1)]


def _mdot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _msub(a, b):
    return [x - y for x, y in zip(a, b)]


def _solve(A, b):
    """Gaussian elimination with partial pivoting on a small mpf system"""
    n = len(b)
    A = [row[:] + [b[i]] for i, row in enumerate(A)]
    for i in range(n):
        piv = max(range(i, n), key=lambda r: abs(A[r][i]))
        A[i], A[piv] = A[piv], A[i]
        for r in range(i + 1, n):
            f = A[r][i] / A[i][i]
            for c in range(i, n + 1):
                A[r][c] -= f * A[i][c]
    x = [mpf(0)] * n
    for i in reversed(range(n)):
        x[i] = (A[i][n] - sum(A[i][c] * x[c] for c in range(i + 1, n))) / A[i][i]
    return x


def closest_point_defects(p, verts, q):
    """-> dict of LENGTHS (floats), each <= eps when q is within eps of the closest point of conv(verts) to p:
    outside  max_v(-lam_v) * (smallest height of the cell), lam the barycentric coordinates of q's foot in the cell's plane (least squares);
    offplane |q - sum lam_v x_v| (0 for M == N up to the solve);
    sum      |1 - sum lam| * diameter (0 by construction of the least-squares form; kept as a guard);
    normal   max_v (p - q).(x_v - q) / (|p - q| + |x_v - q|), 0 where that is negative"""
    with mp.workdps(DPS):
        return _defects(p, verts, q)


def _defects(p, verts, q):
    p, q = _mv(p), _mv(q)
    X = [_mv(v) for v in verts]
    E = [_msub(x, X[0]) for x in X[1:]]
    G = [[_mdot(a, b) for b in E] for a in E]
    xi = _solve(G, [_mdot(e, _msub(q, X[0])) for e in E])
    lam = [1 - sum(xi)] + xi
    foot = [sum(l * x[d] for l, x in zip(lam, X)) for d in range(len(p))]
    off = mp.sqrt(_mdot(_msub(q, foot), _msub(q, foot)))
    # heights: h_v = 1 / |grad lam_v|, grad lam_{k+1} = sum_j Ginv[k][j] E_j, grad lam_0 = - sum of them
    grads = []
    for k in range(len(E)):
        col = _solve(G, [mpf(1) if j == k else mpf(0) for j in range(len(E))])
        grads.append([sum(col[j] * E[j][d] for j in range(len(E))) for d in range(len(p))])
    grads = [[-sum(g[d] for g in grads) for d in range(len(p))]] + grads
    hmin = min(1 / mp.sqrt(_mdot(g, g)) for g in grads)
    diam = max(mp.sqrt(_mdot(_msub(a, b), _msub(a, b))) for a, b in itertools.combinations(X, 2))
    pq = _msub(p, q)
    npq = mp.sqrt(_mdot(pq, pq))
    normal = mpf(0)
    for x in X:
        xq = _msub(x, q)
        den = npq + mp.sqrt(_mdot(xq, xq))
        if den > 0:
            normal = max(normal, _mdot(pq, xq) / den)
    return {"outside": float(max(mpf(0), max(-l for l in lam)) * hmin), "offplane": float(off), "sum": float(abs(1 - sum(lam)) * diam),
            "normal": float(normal), "dist": float(npq)}


# ---- constructed points: one per Voronoi region of a single cell, with the answer known by construction -----------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


def facet_normals(verts):
    """outward unit normals n_v of the facet opposite to vertex v, WITHIN the cell's affine hull (M = 1: the two directions along the segment)"""
    X = np.asarray(verts, dtype=float)
    E = (X[1:] - X[0]).T                      # N x M
    Ginv = np.linalg.inv(E.T @ E)
    grads = (E @ Ginv).T                      # grad lam_{k+1}
    grads = np.vstack([-grads.sum(axis=0), grads])
    return np.array([-_unit(g) for g in grads])


def region_points(verts, off=0.7, lift=0.45):
    """For every non-empty subset S of the vertices (the face of the cell they span): a point p whose closest point is the known q in the
    relative interior of that face: q = the mean of S (weights 1, 2, 3.. normalised), p = q + off * sum of the outward normals of the facets
    that contain S (a point of the face's normal cone) + lift * a unit normal of the cell's affine hull where M < N.
    -> list of (name, p, q, lam, support)"""
    X = np.asarray(verts, dtype=float)
    nv, N = X.shape
    nrm = facet_normals(X)
    extra = np.zeros(N)
    if nv - 1 < N:
        if N == 2:
            d = X[1] - X[0]
            extra = _unit(np.array([-d[1], d[0]]))
        elif N == 3 and nv == 3:
            extra = _unit(np.cross(X[1] - X[0], X[2] - X[0]))
    out = []
    for k in range(1, nv + 1):
        for S in itertools.combinations(range(nv), k):
            w = np.zeros(nv)
            w[list(S)] = np.arange(1, k + 1)
            lam = w / w.sum()
            q = lam @ X
            if k == 1:
                q = X[S[0]].copy()
            cone = [nrm[v] for v in range(nv) if v not in S]   # facet opposite to v contains S iff v is not in S
            p = q + off * np.sum(cone, axis=0) if cone else q.copy()
            p = p + lift * extra
            if k == nv and nv - 1 == N:
                p = q.copy()   # the interior of a cell of full dimension: the point itself
            out.append(("".join(map(str, S)), p, q, lam, S))
    return out
