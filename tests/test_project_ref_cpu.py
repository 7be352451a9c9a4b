"""tests/project_ref.py (the float64 restatement fdapde_project is tested against) certified from first principles in mpmath: on fuzzed cells,
obtuse and thin ones included, the point it returns is in the cell and no vertex lies on the far side of the plane through it normal to p - q
(project_ref.closest_point_defects); and every Voronoi region of one triangle (7) and one tetrahedron (15) is hit by a constructed point whose
answer is known by construction.

The bars (lengths, in units of the cell's diameter e).  The dot products d_i of the region test carry an absolute error of about 4 u D^2, D =
max(|p - x_v|, e), their pairwise products va, vb, vc one of 16 u D^4, and a face coordinate v = vb / (va + vb + vc) divides by (2 area)^2 =
(e h)^2, h the smallest height: the point is off by about 16 u (D / e)^4 (e / h)^2 e.  Points are drawn with D <= 4 e.  Well-shaped cells
(h >= e / 4): 16 u 256 16 = 7e-12 -> bar 1e-11 e.  Thin cells (h >= e / 100): 16 u 256 1e4 = 4.5e-9 -> bar 1e-8 e."""
import numpy as np
import pytest

import project_ref as pr


def _cell(rng, nv, N, kind):
    """a random cell of nv vertices in R^N of diameter 1: 'fat' (smallest height >= 1/4), 'obtuse' (smallest height >= 0.15 and an angle
    between two edges > 100 degrees) or 'thin' (the last vertex 0.02 - 0.04 above a point inside the facet of the others: smallest height in
    [0.01, 0.05])"""
    for _ in range(20000):
        X = rng.uniform(-0.5, 0.5, (nv, N))
        if kind == "thin":
            w = rng.uniform(0.2, 1.0, nv - 1)
            base = (w / w.sum()) @ X[:-1]
            n = rng.standard_normal(N)
            for e in np.linalg.qr((X[1:-1] - X[0]).T)[0].T if nv > 2 else []:
                n = n - (n @ e) * e
            X[-1] = base + rng.uniform(0.02, 0.04) * n / np.linalg.norm(n)
        X = X / max(np.linalg.norm(a - b) for a in X for b in X)
        if nv == 2:
            return X
        hmin = (1.0 / np.linalg.norm(_grads(X), axis=1)).min()
        if (kind == "fat" and hmin >= 0.25) or (kind == "obtuse" and hmin >= 0.15 and _max_angle(X) > 100.0) or (kind == "thin" and 0.01 <= hmin <= 0.05):
            return X
    raise AssertionError("no cell of kind " + kind)


def _grads(X):
    E = (X[1:] - X[0]).T
    g = (E @ np.linalg.inv(E.T @ E)).T
    return np.vstack([-g.sum(axis=0), g])


def _max_angle(X):
    best = 0.0
    for i in range(len(X)):
        for j in range(len(X)):
            for k in range(j + 1, len(X)):
                if i != j and i != k:
                    a, b = X[j] - X[i], X[k] - X[i]
                    best = max(best, np.degrees(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1))))
    return best


SHAPES = [(2, 1), (2, 2), (3, 2), (3, 3), (4, 3)]


# (a segment has one shape)
CASES = [(nv, N, kind) for nv, N in SHAPES for kind in (["fat"] if nv == 2 else ["fat", "obtuse", "thin"])]


@pytest.mark.parametrize("nv,N,kind", CASES)
def test_helper_returns_the_closest_point(nv, N, kind):
    rng = np.random.default_rng(1000 * nv + 10 * N + len(kind))
    bar = 1e-8 if kind == "thin" else 1e-11
    fn = {2: pr.closest_segment, 3: pr.closest_triangle, 4: pr.closest_tetrahedron}[nv]
    worst = {}
    for _ in range(12):
        X = _cell(rng, nv, N, kind)
        P = X.mean(axis=0) + rng.uniform(-2.0, 2.0, (25, N))   # (|p - x_v| <= 2 sqrt(3) + 1/2 < 4 e)
        P[:5] = X.mean(axis=0) + rng.uniform(-0.3, 0.3, (5, N))
        lam, q, d2 = fn(P, *[X[k][None, :] for k in range(nv)])
        assert (lam >= 0).all() and (lam <= 1).all()
        for i in range(len(P)):
            d = pr.closest_point_defects(P[i], X, q[i])
            for k in ("outside", "offplane", "sum", "normal"):
                worst[k] = max(worst.get(k, 0.0), d[k])
            assert abs(np.sqrt(d2[i]) - d["dist"]) <= bar
            assert np.abs(lam[i] @ X - q[i]).max() <= bar
    print(nv, N, kind, worst)
    for k, v in worst.items():
        assert v <= bar, (k, v)


ACUTE3 = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 1.0], [1.5, 3.0, 2.0]])
OBTUSE3 = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.5], [0.5, 0.5, 1.0]])
TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.125, 0.0], [0.25, 1.0, 0.125], [0.125, 0.25, 1.0]])
SEG1 = np.array([[0.25], [1.5]])
SEG2 = np.array([[0.0, 0.5], [2.0, 1.5]])
SINGLE_CELLS = {"seg1": SEG1, "seg2": SEG2, "acute": ACUTE3, "obtuse": OBTUSE3, "tet": TET}


@pytest.mark.parametrize("name", list(SINGLE_CELLS))
def test_every_voronoi_region_is_hit(name):
    X = SINGLE_CELLS[name]
    nv = len(X)
    pts = pr.region_points(X)
    assert len(pts) == 2 ** nv - 1   # 3 for a segment, 7 for a triangle, 15 for a tetrahedron
    fn = {2: pr.closest_segment, 3: pr.closest_triangle, 4: pr.closest_tetrahedron}[nv]
    seen = set()
    for rname, p, q_known, lam_known, S in pts:
        lam, q, d2 = fn(p[None, :], *[X[k][None, :] for k in range(nv)])
        lam, q = lam[0], q[0]
        support = tuple(np.nonzero(lam > 0)[0])
        assert support == S, (rname, lam)
        seen.add(support)
        if len(S) == 1:
            assert np.array_equal(q, X[S[0]]) and lam[S[0]] == 1.0   # a vertex region: the vertex bit for bit
        assert np.abs(q - q_known).max() <= 1e-14 and np.abs(lam - lam_known).max() <= 1e-14   # (coordinates of O(1): a few u)
        assert abs(np.sqrt(d2[0]) - np.linalg.norm(p - q_known)) <= 1e-14
        d = pr.closest_point_defects(p, X, q_known)   # ... and the constructed answer itself is the closest point
        assert max(d["outside"], d["offplane"], d["normal"]) <= 1e-14
    assert len(seen) == 2 ** nv - 1


def test_brute_force_takes_the_lowest_id_on_ties():
    nodes = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    cells = np.array([[1, 3, 2], [0, 1, 2]], dtype=np.int32)
    cell, lam, q, dist = pr.brute_force(nodes, cells, np.array([[1.0, 0.0], [0.5, 0.5], [2.0, 2.0], [-1.0, -1.0]]))
    assert list(cell) == [0, 0, 0, 1] and np.allclose(dist, [0, 0, np.sqrt(2), np.sqrt(2)])
    assert np.array_equal(q[0], [1.0, 0.0]) and np.array_equal(q[2], [1.0, 1.0]) and np.array_equal(q[3], [0.0, 0.0])
