"""The systems, right-hand sides and constants of the Krylov-iterate tests, shared by tests/test_gpu_krylov_iterates.py (which solves them on the GPU) and
tests/test_krylov_ref_cpu.py (which rebuilds them on the CPU and measures the constants) -- plain numpy, nothing of the library."""
import numpy as np

K_CG = (1, 2, 3, 5, 12)
K_BICG = (1, 2, 3)
# c(k): {method: {largest k of the class: (r_cpu measured by tests/test_krylov_ref_cpu.py, c)}}
BOUNDS = {"cg": {5: (19.0, 128.0), 12: (31.0, 128.0)}, "bicgstab": {3: (10.0, 64.0)}}
# relative margin of info.relres against the reference's ||r_k|| / ||bt||: 4 x the checkers' worst, rounded up to a power of two, in units of u
RELRES = {"cg": (52.0, 256.0), "bicgstab": (2.1, 16.0)}
ADV = (0.7, -0.2, 0.4)

# name -> dict(dim, nx, order, dirichlet, react, adv)
SYSTEMS = {
    "sq20": dict(dim=2, nx=20, order=1), "sq60": dict(dim=2, nx=60, order=1), "cube12p2": dict(dim=3, nx=12, order=2),
    "cube25": dict(dim=3, nx=25, order=1), "sq200": dict(dim=2, nx=200, order=1), "sq150free": dict(dim=2, nx=150, order=1, dirichlet=False, react=1.0),
    "cube16": dict(dim=3, nx=16, order=1), "sq24p2": dict(dim=2, nx=24, order=2),
    "cube16adv": dict(dim=3, nx=16, order=1, adv=True), "sq24p2adv": dict(dim=2, nx=24, order=2, adv=True),
    "sq60adv": dict(dim=2, nx=60, order=1, adv=True), "cube25adv": dict(dim=3, nx=25, order=1, adv=True),
    "star": dict(dim=1, nx=2000, order=1),
}
HANDLES = {"sq60": dict(dim=2, nx=60, order=1), "cube12": dict(dim=3, nx=12, order=1)}
HANDLE_COLUMNS = 13   # the most columns a handle test solves at once: batches of 8 and 4 and one column left over
RHS = ("smooth", "cell")
# inputs that were replaced (tests/test_krylov_ref_cpu.py: the cap r_cpu <= 64 and the stop test are conditions on the inputs):
#   sq150free/smooth: without a Dirichlet DOF a smooth right-hand side makes p.At p cancel by ~h^-2, the float64 checkers themselves are 538 u s_i off at
#                     k = 12 -> a random forcing;   cube16/smooth: no residual drop below 0.7 within 12 iterations (0.7001 at k = 1) -> an oscillating one
FORCING = {("sq150free", "smooth"): "random", ("cube16", "smooth"): "oscillating"}
# ... and the one input that has no iteration the stop test could be aimed at (a point source without Dirichlet data: ratios 0.73, 0.81, 0.88, ...)
NO_STOP = {("sq150free", "cell")}
STAR_SEGMENTS = 5   # per arm: with 2 the Jacobi-scaled system is so well clustered that the residual is below float64's floor by iteration 5


def spec_of(name):
    s = dict(dirichlet=True, react=0.4, adv=False)
    s.update(SYSTEMS[name])
    return s


def mesh_of(meshgen, s):
    if s["dim"] == 1:
        return meshgen.star(s["nx"], np.random.default_rng(1).uniform(0.5, 2.0, s["nx"]), k=STAR_SEGMENTS, permute=True)
    return meshgen.unit_square(s["nx"]) if s["dim"] == 2 else meshgen.unit_cube(s["nx"])


def operator_of(mod, s):
    op = -mod.laplacian() + mod.reaction(s["react"])
    if s["adv"]:
        op = op + mod.advection(ADV[:s["dim"]])
    return op


def forcing_of(qn, n_cells, rhs):
    """smooth forcing, or one concentrated in ONE cell (quadrature rows of a cell are consecutive): the Krylov front then leaves s_i = 0 behind"""
    if rhs == "smooth":
        return np.cos(3.0 * qn[:, 0]) + (qn[:, 1] if qn.shape[1] > 1 else 0.0) + 0.5
    if rhs == "oscillating":
        return np.sin(25.0 * qn[:, 0]) * np.cos(31.0 * qn[:, 1])
    if rhs == "random":
        return np.random.default_rng(5).standard_normal(qn.shape[0])
    nq = qn.shape[0] // n_cells
    cent = qn.reshape(n_cells, nq, -1).mean(axis=1)
    lo, hi = qn.min(axis=0), qn.max(axis=0)
    target = lo + np.array([0.37, 0.41, 0.45])[:qn.shape[1]] * (hi - lo)
    j = int(np.argmin(np.linalg.norm(cent - target, axis=1)))
    f = np.zeros(qn.shape[0])
    f[j * nq:(j + 1) * nq] = 1.0e3
    return f


def crafted_values(rowptr, colidx, seed):
    """symmetric off-diagonals +-10^U(-6, 0) on the FEM pattern, diagonal 1.05 sum_j |a_ij|: SPD, mixed signs, six decades inside every block"""
    import scipy.sparse as sp

    n = rowptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    up = rows < colidx
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], int(up.sum())) * 10.0 ** rng.uniform(-6.0, 0.0, int(up.sum()))
    Uu = sp.csr_matrix((v, (rows[up], colidx[up])), shape=(n, n))
    A = (Uu + Uu.T).tocsr()
    d = 1.05 * np.asarray(abs(A).sum(axis=1)).reshape(-1)
    A = (A + sp.diags(d)).tocsr()
    return np.asarray(A[rows, colidx]).reshape(-1)


def handle_rhs(coords, n_cols, seed):
    """columns of a handle test: smooth ones, unit vectors (a Krylov front) and random ones (column j does not depend on n_cols)"""
    n = coords.shape[0]
    rng = np.random.default_rng(seed)
    B = np.zeros((n, n_cols))
    for j in range(n_cols):
        if j % 3 == 0:
            B[:, j] = np.cos((2.0 + j) * coords[:, 0]) + coords[:, 1]
        elif j % 3 == 1:
            B[int(rng.integers(n)), j] = 1.0 + j
        else:
            B[:, j] = rng.standard_normal(n)
    return B


def c_of(method, k):
    for kmax in sorted(BOUNDS[method]):
        if k <= kmax:
            return BOUNDS[method][kmax][1]
    raise KeyError(k)


def pick_stop(rhos, kmax):
    """first k <= kmax whose residual ratio drops below 0.7 of every earlier one -> (k, rtol between them), or None"""
    lo = 1.0
    for k, r in enumerate(rhos[:kmax], start=1):
        if r < 0.7 * lo:
            return k, float(np.sqrt(lo * r))
        lo = min(lo, r)
    return None


STOP_MARGIN = 1.05   # every residual ratio that decides a column's stop iteration is at least 5 % away from the common tolerance


def pick_stop_columns(rhos_of, kmax):
    """ONE tolerance for several columns solved in one call, between two residual ratios of EVERY column.  With k_j the first iteration of column j whose
    ratio is below rtol, the call's margin is the smallest of rtol / rho_{k_j} and rho_m / rtol (m < k_j; 1 at m = 0) over its columns.  pick_stop's 0.7
    cannot be asked of a dozen columns at once (their 150 ratios lie a few per cent apart); STOP_MARGIN = 1.05 is asked instead, which is 10^12 times the
    256 u to which info.relres is held, so no admissible rounding of the residual moves a column's stop iteration.  Candidates are the geometric means of
    neighbours in the sorted union of all ratios; of the admissible ones the tolerance whose stop iterations lie furthest apart is taken (the freeze of a
    finished column while the others go on is what such a call has to get right), then the widest margin.  -> (rtol, [k_j], margin) or None"""
    allr = np.unique(np.concatenate([[1.0]] + [np.asarray(col[:kmax], dtype=float) for col in rhos_of]))
    best = None
    for a, b in zip(allr[:-1], allr[1:]):
        rtol = float(np.sqrt(a * b))
        ks, margin = [], np.inf
        for col in rhos_of:
            k = next((i for i, r in enumerate(col[:kmax], start=1) if r < rtol), None)
            if k is None:
                break
            ks.append(k)
            margin = min([margin, rtol / col[k - 1], 1.0 / rtol] + [r / rtol for r in col[:k - 1]])
        else:
            key = (max(ks) - min(ks), margin)
            if margin >= STOP_MARGIN and key[0] > 0 and (best is None or key > best[0]):
                best = (key, rtol, ks, float(margin))
    return None if best is None else best[1:]
