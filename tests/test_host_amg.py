"""The aggregation set-up's level step as host loops (csrc/host_amg.cpp over the row rules of csrc/amg_rows.h), on the CPU: what the knob `amg_setup_check`
compares the device passes with bit for bit, held here to the numpy restatement (tests/amg_absorb_ref.pairwise, tests/block_amg_ref.galerkin) on the same CSR
in the same numbering.  tests/cpp/host_amg_test.cpp runs host_coarsen without and with absorption on a 5-point Laplacian (24 x 24), a 7-point Laplacian (9^3)
and a seeded random symmetric M-matrix.  Every entry is an integer or a multiple of 1/64, so every Galerkin sum is exact in any order and the comparison is
np.array_equal: both aggregate maps, the coarse pattern and values of both products, a width-4 payload column by column.  Excluded rows, which the
restatement does not know, are checked by their properties and against P^T A P formed by scipy."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_absorb_ref as ab
import block_amg_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "cpp", "host_amg_test.cpp"), os.path.join(ROOT, "fdapde-core_amd", "csrc", "host_amg.cpp")]
WIDTH = 4


def _laplacian(shape):
    """the 5- / 7-point Laplacian on a grid: integer entries"""
    one = [sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m)) for m in shape]
    A = sp.csr_matrix((1, 1))
    for d, L in enumerate(one):
        term = sp.identity(1)
        for e, m in enumerate(shape):
            term = sp.kron(term, L if e == d else sp.identity(m))
        A = term if d == 0 else A + term
    return sp.csr_matrix(A)


def _random_m_matrix(n, seed):
    """symmetric, off-diagonal entries -k / 64, strictly diagonally dominant: about seven entries per row"""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    keep = i < j
    U = sp.csr_matrix((rng.integers(1, 65, keep.sum()) / 64.0, (i[keep], j[keep])), shape=(n, n))
    U.data = np.minimum(U.data, 1.0)   # (duplicates were added up)
    off = U + U.T
    return sp.csr_matrix(sp.diags(np.asarray(off.sum(axis=1)).ravel() + rng.integers(1, 9, n) / 64.0) - off)


MATRICES = {"lap2d_24": lambda: _laplacian((24, 24)), "lap3d_9": lambda: _laplacian((9, 9, 9)), "random_m_400": lambda: _random_m_matrix(400, 7)}
# rows -> aggregates after pass 1 -> after pass 2, (without absorption, with it)
COUNTS = {"lap2d_24": ((310, 170), (266, 116)), "lap3d_9": ((385, 209), (344, 162))}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("host_amg") / "host_amg_test")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", *SRC, "-o", path])
    return path


def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(float), A.shape[0]


def _payload(nnz):
    return np.random.default_rng(11).integers(-128, 129, (nnz, WIDTH)) / 64.0


def _run(exe, tmp_path, rp, ci, a, n, pay, excl=None):
    """host_coarsen on the matrix -> one dict per absorb in (0, 1)"""
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        np.array([n, len(ci), WIDTH, 0 if excl is None else 1], dtype=np.int32).tofile(f)
        for arr, t in ((rp, np.int32), (ci, np.int32), (a, np.float64), (pay, np.float64)):
            np.ascontiguousarray(arr, dtype=t).tofile(f)
        if excl is not None:
            np.ascontiguousarray(excl, dtype=np.uint8).tofile(f)
    outs = [str(tmp_path / f"out{k}.bin") for k in (0, 1)]
    res = subprocess.run([exe, str(src), *outs], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    got = []
    for path in outs:
        raw = np.fromfile(path, dtype=np.uint8)
        pos = 0

        def take(count, t):
            nonlocal pos
            out = raw[pos:pos + count * np.dtype(t).itemsize].view(t)
            assert len(out) == count, "the output file is short"
            pos += count * np.dtype(t).itemsize
            return out

        n1, n2, nnz_t, nnz_n = (int(v) for v in take(4, np.int32))
        d = {"n1": n1, "n2": n2, "agg1": take(n, np.int32), "agg2": take(n1, np.int32), "agg": take(n, np.int32), "mptr": take(n2 + 1, np.int32)}
        d["midx"] = take(int(d["mptr"][-1]), np.int32)
        for name, rows, nnz in (("T", n1, nnz_t), ("N", n2, nnz_n)):
            d[name] = (take(rows + 1, np.int32), take(nnz, np.int32), take(nnz, np.float64), take(WIDTH * nnz, np.float64).reshape(nnz, WIDTH))
        assert pos == len(raw), "the output file is long"
        got.append(d)
    return got


def _same_product(got, rp, ci, vals, agg, nc, n):
    """the device's rule restated (block_amg_ref.galerkin) on [strength values] + the payload's columns, against (rp, ci, a, payload) of the host loops"""
    rp_c, ci_c, out = ar.galerkin(rp, ci, vals, agg, nc, n)
    assert np.array_equal(got[0], rp_c) and np.array_equal(got[1], ci_c)
    assert np.array_equal(got[2], out[0])
    for q in range(WIDTH):
        assert np.array_equal(got[3][:, q], out[1 + q]), f"payload column {q}"
    return rp_c, ci_c, out


@pytest.mark.parametrize("name", list(MATRICES))
def test_host_coarsen_is_the_restatement(exe, tmp_path, name):
    rp, ci, a, n = _csr(MATRICES[name]())
    assert np.all(a * 64 == np.round(a * 64)), "entries are multiples of 1/64: sums are exact in any order"
    pay = _payload(len(ci))
    for absorbing, got in enumerate(_run(exe, tmp_path, rp, ci, a, n, pay)):
        agg1, n1, _ = ab.pairwise(rp, ci, a, n, bool(absorbing))
        assert got["n1"] == n1 and np.array_equal(got["agg1"], agg1)
        rp1, ci1, v1 = _same_product(got["T"], rp, ci, [a] + list(pay.T), agg1, n1, n)
        agg2, n2, _ = ab.pairwise(rp1, ci1, v1[0], n1, bool(absorbing))
        assert got["n2"] == n2 and np.array_equal(got["agg2"], agg2)
        _same_product(got["N"], rp1, ci1, v1, agg2, n2, n1)
        assert np.array_equal(got["agg"], agg2[agg1])
        assert np.array_equal(got["midx"], np.argsort(got["agg"], kind="stable")) and np.array_equal(got["mptr"], np.searchsorted(np.sort(got["agg"]), np.arange(n2 + 1)))
        if name in COUNTS:
            assert (n1, n2) == COUNTS[name][absorbing]


def _prolongation(agg, nc):
    free = np.flatnonzero(agg >= 0)
    return sp.csr_matrix((np.ones(len(free)), (free, agg[free])), shape=(len(agg), nc))


def _is_galerkin(got, P, rp, ci, a, pay, n):
    """(rp, ci, values, payload) of a coarse matrix = P^T A P by scipy: the pattern of P^T |pattern| P, exact values"""
    nc = P.shape[1]
    C = sp.csr_matrix((got[2], got[1], got[0]), shape=(nc, nc))
    pattern = sp.csr_matrix(P.T @ sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n)) @ P)
    pattern.sort_indices()
    assert np.array_equal(pattern.indptr, got[0]) and np.array_equal(pattern.indices, got[1])
    assert np.array_equal(C.toarray(), (P.T @ sp.csr_matrix((a, ci, rp), shape=(n, n)) @ P).toarray())
    for q in range(WIDTH):
        Cq = sp.csr_matrix((got[3][:, q], got[1], got[0]), shape=(nc, nc))
        assert np.array_equal(Cq.toarray(), (P.T @ sp.csr_matrix((pay[:, q], ci, rp), shape=(n, n)) @ P).toarray()), f"payload column {q}"


@pytest.mark.parametrize("name", ["lap2d_24", "random_m_400"])
def test_host_coarsen_with_excluded_rows(exe, tmp_path, name):
    rp, ci, a, n = _csr(MATRICES[name]())
    if name == "lap2d_24":   # the grid's boundary, as a Dirichlet problem excludes it
        ij = np.indices((24, 24)).reshape(2, -1)
        excl = ((ij == 0) | (ij == 23)).any(axis=0)
    else:
        excl = np.random.default_rng(3).random(n) < 0.2
    free = np.flatnonzero(~excl)
    pay = _payload(len(ci))
    for absorbing, got in enumerate(_run(exe, tmp_path, rp, ci, a, n, pay, excl.astype(np.uint8))):
        n1, n2, agg1, agg2, agg = got["n1"], got["n2"], got["agg1"], got["agg2"], got["agg"]
        assert np.all(agg1[excl] == -1) and np.all(agg[excl] == -1)
        # the free rows' aggregates are exactly 0 .. nc - 1, on both passes and composed
        assert np.array_equal(np.unique(agg1[free]), np.arange(n1)) and np.array_equal(np.unique(agg2), np.arange(n2)) and np.array_equal(np.unique(agg[free]), np.arange(n2))
        assert np.array_equal(agg[free], agg2[agg1[free]])
        if not absorbing:
            assert np.bincount(agg1[free]).max() <= 2 and np.bincount(agg2).max() <= 2
        # members: the free rows, each once, grouped by aggregate, ascending within it; no excluded row
        assert np.array_equal(got["midx"], free[np.argsort(agg[free], kind="stable")])
        assert np.array_equal(got["mptr"], np.searchsorted(np.sort(agg[free]), np.arange(n2 + 1)))
        P1, P2 = _prolongation(agg1, n1), _prolongation(agg2, n2)
        _is_galerkin(got["T"], P1, rp, ci, a, pay, n)
        rp1, ci1, a1, pay1 = got["T"]
        _is_galerkin(got["N"], P2, rp1.astype(np.int64), ci1.astype(np.int64), a1, pay1, n1)
