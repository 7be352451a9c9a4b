"""ctypes binding of the C ABI in include/fdapde_hip.h (libfdapde_hip.so).

Plumbing for tests/ and bench.py only: the product's host side is the header-only C++20 facade in
include/fdapde_amd/ (the reference is a C++ library).  There is no CPU fallback here -- if the shared library is
missing, import fails loudly; if a context has no device, compute calls raise FdapdeError(ENODEVICE).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FDAPDE_HIP_LIB") or os.path.join(_HERE, "lib", "libfdapde_hip.so")   # (override: A/B builds of tools/)

OK, EINVAL, ENOMEM, ENODEVICE, EHIP, ENOTINIT, ENOCONV, EUNSUPPORTED, ERCCL = range(9)
LAPLACIAN, DIFFUSION, ADVECTION, REACTION, DT = range(5)
SOLVER_AUTO, SOLVER_CG, SOLVER_BICGSTAB, SOLVER_CG_SR, SOLVER_CG_FUSED, SOLVER_GMRES, SOLVER_DENSE, SOLVER_PMG, SOLVER_AMG, SOLVER_BLOCK_AMG = range(10)
SOLVER_KRON_AMG = 10
ASSEMBLY_ROWS, ASSEMBLY_ATOMIC, ASSEMBLY_COLOURED, ASSEMBLY_PARTITIONED, ASSEMBLY_WAVE = range(5)
MAT_STIFF, MAT_MASS = 0, 1


class Term(C.Structure):
    _fields_ = [("kind", C.c_int32), ("space_varying", C.c_int32), ("coef", C.c_double), ("cst", C.c_double * 9),
                ("data", C.POINTER(C.c_double))]


class Options(C.Structure):
    _fields_ = [("method", C.c_int32), ("maxit", C.c_int32), ("rtol", C.c_double), ("assembly", C.c_int32),
                ("check_every", C.c_int32), ("time_spmv", C.c_int32)]


class Info(C.Structure):
    _fields_ = [("iters", C.c_int32), ("converged", C.c_int32), ("relres", C.c_double), ("t_assemble_ms", C.c_double),
                ("t_solve_ms", C.c_double), ("t_setup_ms", C.c_double), ("spmv_avg_ms", C.c_double), ("spmv_timed", C.c_int32),
                ("method_used", C.c_int32), ("persistent", C.c_int32), ("gather_avg_ms", C.c_double), ("update_avg_ms", C.c_double),
                ("spmv_mean_ms", C.c_double), ("launch_ms", C.c_double)]


# every symbol include/fdapde_hip.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "fdapde_abi_version", "fdapde_device_count", "fdapde_ctx_create", "fdapde_ctx_destroy", "fdapde_last_error",
    "fdapde_status_string", "fdapde_mesh_upload", "fdapde_dofs_build", "fdapde_dofs_get", "fdapde_dofs_set_boundary", "fdapde_sizes",
    "fdapde_pattern_get", "fdapde_quadrature_nodes", "fdapde_set_operator", "fdapde_set_forcing", "fdapde_set_dirichlet",
    "fdapde_init", "fdapde_assemble_operator", "fdapde_solver_prepare", "fdapde_solve", "fdapde_matrix_values", "fdapde_lump", "fdapde_force", "fdapde_solution",
    "fdapde_info_get", "fdapde_spmv", "fdapde_bench_spmv", "fdapde_tune", "fdapde_stream", "fdapde_synchronize",
    "fdapde_comm_unique_id", "fdapde_comm_init", "fdapde_halo_setup", "fdapde_solve_parabolic",
    "fdapde_lin_compute", "fdapde_lin_solve", "fdapde_eval_pointwise", "fdapde_project", "fdapde_cell_integrals", "fdapde_comm_init_callback", "fdapde_comm_set_exchange_callback", "fdapde_halo_setup_peers",
    "fdapde_solver_layout", "fdapde_topology_build", "fdapde_topology_get", "fdapde_comm_allreduce", "fdapde_comm_library", "fdapde_solver_layout_kind", "fdapde_solver_layout_partition", "fdapde_solver_trace", "fdapde_solve_reuse_count", "fdapde_rowdist_setup", "fdapde_ctx_clone", "fdapde_comm_count",
    "fdapde_ctx_create_multi", "fdapde_ctx_devices", "fdapde_partition_build", "fdapde_partition_sizes", "fdapde_partition_get", "fdapde_partition_whole",
    "fdapde_partition_peers",
    "fdapde_block_compute", "fdapde_block_solve", "fdapde_block_spmv", "fdapde_block_bench_spmv", "fdapde_gram_pointwise",
    "fdapde_block_set_obs", "fdapde_block_obs_info", "fdapde_block_obs_amg_levels",
    "fdapde_kron_compute", "fdapde_kron_solve", "fdapde_kron_spmv", "fdapde_kron_bench_spmv",
    "fdapde_kron_set_obs", "fdapde_kron_obs_info",
    "fdapde_kron_amg_hierarchy", "fdapde_kron_amg_aggregates",
    "fdapde_amg_hierarchy", "fdapde_amg_aggregates", "fdapde_amg_order", "fdapde_amg_damping", "fdapde_amg_cols_trace",
]
AMG_OF_SOLVE, AMG_OF_HANDLE, AMG_OF_BLOCK = 0, 1, 2   # `which` of fdapde_amg_hierarchy
PARTITION_ROWDIST, PARTITION_ELEMENTS = 0, 1

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() or `make -C fdapde-core_amd/csrc`. "
                              "There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        lib.fdapde_last_error.restype = C.c_char_p
        lib.fdapde_status_string.restype = C.c_char_p
        lib.fdapde_stream.restype = C.c_void_p
        lib.fdapde_comm_library.restype = C.c_char_p
        lib.fdapde_ctx_destroy.restype = None
        _lib = lib
    return _lib


class FdapdeError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"[status {status}] {msg}")
        self.status = status


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _bp(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class Operator:
    """Left-to-right sum of scaled leaves, mirroring the reference's operator algebra
    (fdaPDE/pde/differential_expressions.h): -laplacian(), a + b, a - b, 2.0 * a."""

    def __init__(self, terms=None):
        self.terms = list(terms or [])  # (kind, coef, const | None, data | None)

    def __neg__(self):
        return Operator([(k, -c, cst, d) for (k, c, cst, d) in self.terms])

    def __add__(self, o):
        return Operator(self.terms + o.terms)

    def __sub__(self, o):
        return Operator(self.terms + (-o).terms)

    def __rmul__(self, s):
        return Operator([(k, float(s) * c, cst, d) for (k, c, cst, d) in self.terms])

    @property
    def is_symmetric(self):
        return all(k != ADVECTION for (k, _, _, _) in self.terms)

    def c_terms(self):
        arr = (Term * len(self.terms))()
        keep = []
        for t, (k, c, cst, d) in zip(arr, self.terms):
            t.kind, t.coef, t.space_varying = k, c, 0 if d is None else 1
            if cst is not None:
                for i, v in enumerate(np.asarray(cst, dtype=float).reshape(-1)):
                    t.cst[i] = v
            if d is not None:
                dd = np.ascontiguousarray(d, dtype=float)
                keep.append(dd)
                t.data = _dp(dd)
        return arr, keep


def laplacian():
    return Operator([(LAPLACIAN, 1.0, None, None)])


def diffusion(K):
    return Operator([(DIFFUSION, 1.0, np.asarray(K, dtype=float), None)])


def diffusion_field(Kq):
    return Operator([(DIFFUSION, 1.0, None, np.asarray(Kq, dtype=float))])


def advection(b):
    return Operator([(ADVECTION, 1.0, np.asarray(b, dtype=float), None)])


def advection_field(bq):
    return Operator([(ADVECTION, 1.0, None, np.asarray(bq, dtype=float))])


def reaction(c):
    return Operator([(REACTION, 1.0, np.asarray([c], dtype=float), None)])


def reaction_field(cq):
    return Operator([(REACTION, 1.0, None, np.asarray(cq, dtype=float))])


def dt():
    return Operator([(DT, 1.0, None, None)])


class Context:
    """One fdapde_ctx.  device=None -> host-only context (numbering / pattern queries only)."""

    def __init__(self, device=0, devices=None):
        """devices=[d0, d1, ...]: ONE context over several devices (fdapde_ctx_create_multi; a device may be named several times)"""
        self.lib = load()
        self._ctx = C.c_void_p()
        if devices is not None:
            dv = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = self.lib.fdapde_ctx_create_multi(dv, len(devices), C.byref(self._ctx))
        else:
            rc = self.lib.fdapde_ctx_create(-1 if device is None else int(device), C.byref(self._ctx))
        if rc != OK:
            raise FdapdeError(rc, self.lib.fdapde_status_string(rc).decode())
        self.M = self.N = 0
        self.n_cells = self.n_nodes = 0

    def devices(self):
        """-> dict(devices=[...], form=0 row-distributed | 1 element partition | -1 single device, t_partition_ms, t_rank_setup_ms)"""
        n = C.c_int32()
        self._check(self.lib.fdapde_ctx_devices(self._ctx, C.byref(n), None, None, None, None))
        dv = (C.c_int32 * n.value)()
        form, tp, tr = C.c_int32(), C.c_double(), C.c_double()
        self._check(self.lib.fdapde_ctx_devices(self._ctx, C.byref(n), dv, C.byref(form), C.byref(tp), C.byref(tr)))
        return dict(devices=list(dv), form=form.value, t_partition_ms=tp.value, t_rank_setup_ms=tr.value)

    # ---- the device-side partitioner (rank processes: every process partitions the whole mesh on its own device and takes its share)
    def partition_build(self, world, form=PARTITION_ROWDIST):
        self._check(self.lib.fdapde_partition_build(self._ctx, int(world), int(form)))
        self._part_world = int(world)

    def partition_get(self, rank):
        """-> dict(nodes (n, N), cells (m, M + 1) local ids, boundary, l2g (global node ids, ascending), cell_ids, owner (rank owning each local node))"""
        nn, nc = C.c_int64(), C.c_int64()
        self._check(self.lib.fdapde_partition_sizes(self._ctx, int(rank), C.byref(nn), C.byref(nc)))
        nn, nc = nn.value, nc.value
        nodes = np.zeros(nn * self.N)
        cells = np.zeros((nc, self.M + 1), dtype=np.int32)
        bnd = np.zeros(nn, dtype=np.uint8)
        l2g, cids, own = np.zeros(nn, dtype=np.int64), np.zeros(nc, dtype=np.int64), np.zeros(nn, dtype=np.int32)
        self._check(self.lib.fdapde_partition_get(self._ctx, int(rank), _dp(nodes), _ip(cells), _bp(bnd), l2g.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  cids.ctypes.data_as(C.POINTER(C.c_int64)), _ip(own)))
        return dict(nodes=np.ascontiguousarray(nodes.reshape(self.N, nn).T), cells=cells, boundary=bnd, l2g=l2g, cell_ids=cids, owner=own)

    def partition_whole(self):
        """-> (rank of every cell, owner of every node, bit mask of the ranks whose sub-mesh holds a node)"""
        part = np.zeros(self.n_cells, dtype=np.int32)
        own = np.zeros(self.n_nodes, dtype=np.int32)
        mask = np.zeros(self.n_nodes, dtype=np.uint64)
        self._check(self.lib.fdapde_partition_whole(self._ctx, _ip(part), _ip(own), mask.ctypes.data_as(C.POINTER(C.c_uint64))))
        return part, own, mask

    def partition_peers(self, rank):
        """element form, P1: (peer_rank, peer_off, peer_dof, owned) for halo_setup_peers"""
        npeers, nshared = C.c_int32(), C.c_int64()
        self._check(self.lib.fdapde_partition_peers(self._ctx, int(rank), C.byref(npeers), None, None, None, None, C.byref(nshared)))
        nn = C.c_int64()
        self._check(self.lib.fdapde_partition_sizes(self._ctx, int(rank), C.byref(nn), None))
        pr = np.zeros(max(npeers.value, 1), dtype=np.int32)
        po = np.zeros(npeers.value + 1, dtype=np.int64)
        pd = np.zeros(max(nshared.value, 1), dtype=np.int32)
        owned = np.zeros(nn.value, dtype=np.uint8)
        self._check(self.lib.fdapde_partition_peers(self._ctx, int(rank), C.byref(npeers), _ip(pr), po.ctypes.data_as(C.POINTER(C.c_int64)), _ip(pd), _bp(owned),
                                                    C.byref(nshared)))
        return pr[:npeers.value], po, pd[:nshared.value], owned

    def clone(self):
        """fdapde_ctx_clone: an independent context with the same problem, assembled state and solution"""
        other = Context.__new__(Context)
        other.lib, other._ctx = self.lib, C.c_void_p()
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("lib", "_ctx")})
        self._check(self.lib.fdapde_ctx_clone(self._ctx, C.byref(other._ctx)))
        return other

    def close(self):
        if self._ctx:
            self.lib.fdapde_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise FdapdeError(rc, self.lib.fdapde_last_error(self._ctx).decode() or self.lib.fdapde_status_string(rc).decode())

    # ---- domain / space
    def mesh_upload(self, nodes, cells, boundary):
        """nodes (n_nodes, N) any order; cells (n_cells, M+1) int32 0-based; boundary (n_nodes,) 0/1.  (M, N) comes from the shapes: 2-column
        cells are segments (M = 1) of an interval (nodes (n_nodes,) or (n_nodes, 1)) or of a network in the plane (nodes (n_nodes, 2))"""
        nodes = np.asarray(nodes, dtype=float)
        if nodes.ndim == 1:
            nodes = nodes.reshape(-1, 1)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        boundary = np.ascontiguousarray(boundary, dtype=np.uint8).reshape(-1)
        colmajor = np.ascontiguousarray(nodes.T).reshape(-1)
        self.M, self.N = cells.shape[1] - 1, nodes.shape[1]
        self.n_nodes, self.n_cells = nodes.shape[0], cells.shape[0]
        self._check(self.lib.fdapde_mesh_upload(self._ctx, self.M, self.N, C.c_int64(self.n_nodes), _dp(colmajor),
                                                C.c_int64(self.n_cells), _ip(cells), _bp(boundary)))

    def topology(self):
        """Triangulation topology tables (device-built): dict of neighbors, cell_facets, facet_nodes, facet_cells, facet_boundary
        and, for tetrahedra, edge_nodes, edge_boundary, face_edges"""
        nf, ne = C.c_int64(), C.c_int64()
        self._check(self.lib.fdapde_topology_build(self._ctx, C.byref(nf), C.byref(ne)))
        M, nc, nf, ne = self.M, self.n_cells, nf.value, ne.value
        t = dict(neighbors=np.zeros((nc, M + 1), np.int32), cell_facets=np.zeros((nc, M + 1), np.int32), facet_nodes=np.zeros((nf, M), np.int32),
                 facet_cells=np.zeros((nf, 2), np.int32), facet_boundary=np.zeros(nf, np.uint8))
        if M == 3:
            t.update(edge_nodes=np.zeros((ne, 2), np.int32), edge_boundary=np.zeros(ne, np.uint8), face_edges=np.zeros((nf, 3), np.int32))
        self._check(self.lib.fdapde_topology_get(self._ctx, _ip(t["neighbors"]), _ip(t["cell_facets"]), _ip(t["facet_nodes"]),
                                                 _ip(t["facet_cells"]), _bp(t["facet_boundary"]),
                                                 _ip(t["edge_nodes"]) if M == 3 else None, _bp(t["edge_boundary"]) if M == 3 else None,
                                                 _ip(t["face_edges"]) if M == 3 else None))
        return t

    def dofs_build(self, order):
        nd = C.c_int64()
        self._check(self.lib.fdapde_dofs_build(self._ctx, int(order), C.byref(nd)))
        self.order = order
        return nd.value

    def sizes(self):
        nd, nnz, ne = C.c_int64(), C.c_int64(), C.c_int64()
        nb, nq = C.c_int32(), C.c_int32()
        self._check(self.lib.fdapde_sizes(self._ctx, C.byref(nd), C.byref(nnz), C.byref(nb), C.byref(nq), C.byref(ne)))
        return dict(n_dofs=nd.value, nnz=nnz.value, n_basis=nb.value, n_quadrature=nq.value, n_edges=ne.value)

    def dofs_get(self):
        s = self.sizes()
        dofs = np.zeros((self.n_cells, s["n_basis"]), dtype=np.int32)
        bnd = np.zeros(s["n_dofs"], dtype=np.uint8)
        coords = np.zeros(self.N * s["n_dofs"])
        self._check(self.lib.fdapde_dofs_get(self._ctx, _ip(dofs), _bp(bnd), _dp(coords)))
        return dofs, bnd, np.ascontiguousarray(coords.reshape(self.N, s["n_dofs"]).T)

    def dofs_set_boundary(self, bnd):
        bnd = np.ascontiguousarray(bnd, dtype=np.uint8)
        assert bnd.size == self.sizes()["n_dofs"]
        self._check(self.lib.fdapde_dofs_set_boundary(self._ctx, _bp(bnd)))

    def pattern_get(self):
        s = self.sizes()
        rowptr = np.zeros(s["n_dofs"] + 1, dtype=np.int32)
        colidx = np.zeros(s["nnz"], dtype=np.int32)
        self._check(self.lib.fdapde_pattern_get(self._ctx, _ip(rowptr), _ip(colidx)))
        return rowptr, colidx

    def quadrature_nodes(self):
        s = self.sizes()
        rows = s["n_quadrature"] * self.n_cells
        out = np.zeros(self.N * rows)
        self._check(self.lib.fdapde_quadrature_nodes(self._ctx, _dp(out)))
        return np.ascontiguousarray(out.reshape(self.N, rows).T)

    # ---- problem data
    def set_operator(self, op: Operator):
        terms, keep = op.c_terms()
        self._check(self.lib.fdapde_set_operator(self._ctx, len(op.terms), terms))

    def set_forcing(self, f_q):
        if f_q is None:
            self._check(self.lib.fdapde_set_forcing(self._ctx, None, 0))
            self._force_cols = 1
            return
        f = np.asarray(f_q, dtype=float)
        ncols = 1 if f.ndim == 1 else f.shape[1]
        self._force_cols = ncols
        flat = np.ascontiguousarray(f.reshape(f.shape[0], ncols).T).reshape(-1)  # column-major
        self._check(self.lib.fdapde_set_forcing(self._ctx, _dp(flat), ncols))

    def set_dirichlet(self, g):
        if g is None:
            self._check(self.lib.fdapde_set_dirichlet(self._ctx, None))
        else:
            g = np.ascontiguousarray(g, dtype=float).reshape(-1)
            self._check(self.lib.fdapde_set_dirichlet(self._ctx, _dp(g)))

    # ---- compute
    def init(self, assembly=ASSEMBLY_ROWS):
        opt = Options(method=0, maxit=0, rtol=0.0, assembly=assembly, check_every=0, time_spmv=0)
        self._check(self.lib.fdapde_init(self._ctx, C.byref(opt)))

    def assemble_operator(self, which, op: Operator, assembly=ASSEMBLY_ROWS):
        terms, keep = op.c_terms()
        self._check(self.lib.fdapde_assemble_operator(self._ctx, which, len(op.terms), terms, assembly))

    def solver_prepare(self, with_dirichlet=True):
        self._check(self.lib.fdapde_solver_prepare(self._ctx, 1 if with_dirichlet else 0))

    def solve(self, method=SOLVER_AUTO, rtol=1e-10, maxit=0, check_every=0, raise_on_noconv=True, time_spmv=0):
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=check_every, time_spmv=time_spmv)
        info = Info()
        rc = self.lib.fdapde_solve(self._ctx, C.byref(opt), C.byref(info))
        if rc != OK and (raise_on_noconv or rc != ENOCONV):
            self._check(rc)
        return info

    def solve_parabolic(self, times, initial_condition, dirichlet=None, method=SOLVER_AUTO, rtol=1e-10, maxit=0):
        """FEMLinearParabolicSolver::solve; dirichlet (n_dofs, n_times) or None -> solution (n_dofs, n_times), Info"""
        times = np.asarray(times, dtype=float).reshape(-1)
        m, nd = times.size, self.sizes()["n_dofs"]
        u0 = np.ascontiguousarray(initial_condition, dtype=float).reshape(-1)
        g = None if dirichlet is None else np.ascontiguousarray(np.asarray(dirichlet, dtype=float).T).reshape(-1)
        out = np.zeros(nd * m)
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
        info = Info()
        self._check(self.lib.fdapde_solve_parabolic(self._ctx, C.byref(opt), int(m), C.c_double(times[1] - times[0]), _dp(u0),
                                                    None if g is None else _dp(g), _dp(out), C.byref(info)))
        return np.ascontiguousarray(out.reshape(m, nd).T), info

    def lin_compute(self, which=MAT_STIFF, values=None, symmetric=False):
        """fdapde::SparseLU::compute: 'factor once'"""
        v = None if values is None else np.ascontiguousarray(values, dtype=float)
        self._check(self.lib.fdapde_lin_compute(self._ctx, which, None if v is None else _dp(v), 1 if symmetric else 0))

    def lin_solve(self, b, method=SOLVER_AUTO, rtol=1e-10, check_every=0, maxit=0, raise_on_noconv=True):
        """fdapde::SparseLU::solve(b); b (n_dofs,) or (n_dofs, n_rhs).  raise_on_noconv=False: FDAPDE_ENOCONV is reported through
        info.converged only, and x holds the last iterate of every column (as after solve)"""
        b = np.asarray(b, dtype=float)
        one = b.ndim == 1
        B = b.reshape(b.shape[0], -1)
        flat = np.ascontiguousarray(B.T).reshape(-1)
        out = np.zeros_like(flat)
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=check_every, time_spmv=0)
        info = Info()
        rc = self.lib.fdapde_lin_solve(self._ctx, C.byref(opt), _dp(flat), B.shape[1], _dp(out), C.byref(info))
        if rc != OK and (raise_on_noconv or rc != ENOCONV):
            self._check(rc)
        X = np.ascontiguousarray(out.reshape(B.shape[1], B.shape[0]).T)
        return (X[:, 0] if one else X), info

    # ---- 2 x 2 block systems on the FEM pattern (SparseBlockMatrix<double,2,2> under fdapde::SparseLU): the smoothing system's handle
    def block_compute(self, a11, a12, a21, a22, symmetric=False):
        """fdapde_block_compute: four blocks of nnz values each, aligned with pattern_get(); None = a zero block"""
        nnz = self.sizes()["nnz"]
        keep = []
        for a in (a11, a12, a21, a22):
            if a is None:
                keep.append(None)
                continue
            v = np.ascontiguousarray(a, dtype=float).reshape(-1)
            if v.size != nnz:
                raise ValueError(f"block_compute(): a block holds {v.size} values, the pattern has {nnz} entries")
            keep.append(v)
        self._check(self.lib.fdapde_block_compute(self._ctx, *[None if v is None else _dp(v) for v in keep], 1 if symmetric else 0))

    def block_solve(self, b, method=SOLVER_AUTO, rtol=1e-10, maxit=0, raise_on_noconv=True):
        """fdapde_block_solve: b (2 n_dofs,) or (2 n_dofs, n_rhs), stacked [first block row; second block row] -> (x, Info).
        raise_on_noconv=False: FDAPDE_ENOCONV is reported through info.converged only, x holds the last iterate of every column"""
        b = np.asarray(b, dtype=float)
        one = b.ndim == 1
        B = b.reshape(b.shape[0], -1)
        flat = np.ascontiguousarray(B.T).reshape(-1)
        out = np.zeros_like(flat)
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
        info = Info()
        rc = self.lib.fdapde_block_solve(self._ctx, C.byref(opt), _dp(flat), B.shape[1], _dp(out), C.byref(info))
        if rc != OK and (raise_on_noconv or rc != ENOCONV):
            self._check(rc)
        X = np.ascontiguousarray(out.reshape(B.shape[1], B.shape[0]).T)
        return (X[:, 0] if one else X), info

    def block_solve_inplace(self, bx, method=SOLVER_AUTO, rtol=1e-10, maxit=0):
        """fdapde_block_solve with x = b: bx (2 n_dofs, n_rhs) Fortran-ordered float64 is overwritten by the solutions -> Info"""
        assert bx.dtype == np.float64 and bx.ndim == 2 and bx.flags.f_contiguous
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
        info = Info()
        self._check(self.lib.fdapde_block_solve(self._ctx, C.byref(opt), _dp(bx), bx.shape[1], _dp(bx), C.byref(info)))
        return info

    def block_spmv(self, x):
        """y = A x with the unscaled blocks, stacked vectors of 2 n_dofs"""
        x = np.ascontiguousarray(x, dtype=float).reshape(-1)
        if x.size != 2 * self.sizes()["n_dofs"]:
            raise ValueError("block_spmv(): x must hold 2 n_dofs values")
        y = np.zeros_like(x)
        self._check(self.lib.fdapde_block_spmv(self._ctx, _dp(x), _dp(y)))
        return y

    def block_bench_spmv(self, reps=50):
        """(average ms of the Krylov stage's operator -- k_block_spmv on the scaled blocks and, with a data term live, its two products --, algorithmic bytes
        per application)"""
        ms, by = C.c_double(), C.c_double()
        self._check(self.lib.fdapde_block_bench_spmv(self._ctx, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def block_set_obs(self, psi, weights=None, scale=-1.0):
        """fdapde_block_set_obs: the handle's matrix becomes A + scale [Psi^T W Psi, 0; 0, 0], the term kept factored.  psi: a scipy.sparse matrix
        (n_obs x n_dofs; duplicates summed, columns sorted), a triple (rowptr, colidx, values) handed to the library as it is, or None (clears the term).
        weights: one per row, or None (W = I)"""
        if psi is None:
            self._check(self.lib.fdapde_block_set_obs(self._ctx, C.c_int64(0), None, None, None, None, C.c_double(scale)))
            return
        if isinstance(psi, (tuple, list)):
            rp, ci, v = psi
        else:
            m = psi.tocsr().copy()
            m.sum_duplicates()
            m.sort_indices()
            if m.shape[1] != self.sizes()["n_dofs"]:
                raise ValueError("block_set_obs(): Psi needs n_dofs columns")
            rp, ci, v = m.indptr, m.indices, m.data
        rp = np.ascontiguousarray(rp, dtype=np.int64).reshape(-1)
        ci = np.ascontiguousarray(ci, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(v, dtype=float).reshape(-1)
        if rp.size < 1 or ci.size != v.size or (rp.size > 1 and rp.max() > ci.size):
            raise ValueError("block_set_obs(): rowptr / colidx / values do not fit together")
        n_obs = rp.size - 1
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=float).reshape(-1)
            if w.size != n_obs:
                raise ValueError("block_set_obs(): one weight per row of Psi")
        self._check(self.lib.fdapde_block_set_obs(self._ctx, C.c_int64(n_obs), rp.ctypes.data_as(C.POINTER(C.c_int64)), _ip(ci), _dp(v),
                                                  None if w is None else _dp(w), C.c_double(scale)))

    def block_obs_info(self):
        """fdapde_block_obs_info -> dict(n_obs, nnz, team_rows, team_cols): the live data term's sizes and the lanes per row of Psi / of Psi^T"""
        n_obs, nnz, tr, tc = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        self._check(self.lib.fdapde_block_obs_info(self._ctx, C.byref(n_obs), C.byref(nnz), C.byref(tr), C.byref(tc)))
        return {"n_obs": n_obs.value, "nnz": nnz.value, "team_rows": tr.value, "team_cols": tc.value}

    def block_amg_obs_levels(self):
        """fdapde_block_obs_amg_levels -> dict(nnz, longest_row, team_rows, team_cols: per level of the live block hierarchy that carries the data term -- knob
        block_amg_obs = 1).  FdapdeError(ENOTINIT) where no live hierarchy carries a term"""
        nl = C.c_int32()
        self._check(self.lib.fdapde_block_obs_amg_levels(self._ctx, 0, C.byref(nl), None, None, None, None))
        nnz = np.zeros(nl.value, dtype=np.int64)
        lr, tr, tc = (np.zeros(nl.value, dtype=np.int32) for _ in range(3))
        self._check(self.lib.fdapde_block_obs_amg_levels(self._ctx, nl.value, C.byref(nl), nnz.ctypes.data_as(C.POINTER(C.c_int64)), _ip(lr), _ip(tr), _ip(tc)))
        return dict(nnz=[int(z) for z in nnz], longest_row=[int(z) for z in lr], team_rows=[int(z) for z in tr], team_cols=[int(z) for z in tc])

    # ---- Kronecker-sum operators sum_k T_k (x) S_k on the FEM pattern (the reference's Kronecker(A, B) under fdapde::SparseLU): the space-time systems' handle
    def kron_compute(self, terms, symmetric=False):
        """fdapde_kron_compute: terms = [(T, S_values), ...], T dense q x q, S_values nnz values aligned with pattern_get().  Terms that hand over the
        SAME S_values object share one spatial factor.  q and the number of terms are checked by the library (EINVAL); a None factor goes through as NULL"""
        nnz = self.sizes()["nnz"]
        terms = list(terms)
        q = 0
        for T, _ in terms:
            if T is not None:
                q = int(np.asarray(T).shape[0]) if np.asarray(T).ndim == 2 else 0
                break
        keep_t, keep_s, by_id = [], [], {}
        for T, S in terms:
            if T is None:
                keep_t.append(None)
            else:
                t = np.asfortranarray(np.asarray(T, dtype=float))
                if t.ndim != 2 or t.shape != (q, q):
                    raise ValueError("kron_compute(): every T must be q x q")
                keep_t.append(t)
            if S is None:
                keep_s.append(None)
            else:
                if id(S) not in by_id:
                    v = np.ascontiguousarray(S, dtype=float).reshape(-1)
                    if v.size != nnz:
                        raise ValueError(f"kron_compute(): a spatial factor holds {v.size} values, the pattern has {nnz} entries")
                    by_id[id(S)] = v
                keep_s.append(by_id[id(S)])
        PP = C.POINTER(C.c_double) * max(1, len(terms))
        tp = PP(*[_dp(t) if t is not None else C.POINTER(C.c_double)() for t in keep_t])
        sp_ = PP(*[_dp(s) if s is not None else C.POINTER(C.c_double)() for s in keep_s])
        self._check(self.lib.fdapde_kron_compute(self._ctx, q, len(terms), tp, sp_, 1 if symmetric else 0))
        self._kron_q = q

    def _kron_rows(self):
        return getattr(self, "_kron_q", 0) * self.sizes()["n_dofs"]

    def kron_solve(self, b, method=SOLVER_AUTO, rtol=1e-10, maxit=0, raise_on_noconv=True):
        """fdapde_kron_solve: b (q n_dofs,) or (q n_dofs, n_rhs) in the Kronecker order (index r n_dofs + i) -> (x, Info).
        raise_on_noconv=False: FDAPDE_ENOCONV is reported through info.converged only, x holds the last iterate of every column"""
        b = np.asarray(b, dtype=float)
        one = b.ndim == 1
        B = b.reshape(b.shape[0], -1)
        if getattr(self, "_kron_q", 0) and B.shape[0] != self._kron_rows():
            raise ValueError("kron_solve(): b must hold q n_dofs rows")
        flat = np.ascontiguousarray(B.T).reshape(-1)
        out = np.zeros_like(flat)
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
        info = Info()
        rc = self.lib.fdapde_kron_solve(self._ctx, C.byref(opt), _dp(flat), B.shape[1], _dp(out), C.byref(info))
        if rc != OK and (raise_on_noconv or rc != ENOCONV):
            self._check(rc)
        X = np.ascontiguousarray(out.reshape(B.shape[1], B.shape[0]).T)
        return (X[:, 0] if one else X), info

    def kron_solve_inplace(self, bx, method=SOLVER_AUTO, rtol=1e-10, maxit=0):
        """fdapde_kron_solve with x = b: bx (q n_dofs, n_rhs) Fortran-ordered float64 is overwritten by the solutions -> Info"""
        assert bx.dtype == np.float64 and bx.ndim == 2 and bx.flags.f_contiguous
        if getattr(self, "_kron_q", 0) and bx.shape[0] != self._kron_rows():
            raise ValueError("kron_solve_inplace(): bx must hold q n_dofs rows")
        opt = Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
        info = Info()
        self._check(self.lib.fdapde_kron_solve(self._ctx, C.byref(opt), _dp(bx), bx.shape[1], _dp(bx), C.byref(info)))
        return info

    def kron_spmv(self, x):
        """y = A x, vectors of q n_dofs in the Kronecker order"""
        x = np.ascontiguousarray(x, dtype=float).reshape(-1)
        if getattr(self, "_kron_q", 0) and x.size != self._kron_rows():
            raise ValueError("kron_spmv(): x must hold q n_dofs values")
        y = np.zeros_like(x)
        self._check(self.lib.fdapde_kron_spmv(self._ctx, _dp(x), _dp(y)))
        return y

    def kron_bench_spmv(self, reps=50):
        """(average ms of the Krylov stage's operator D^-1 A, algorithmic bytes per application)"""
        ms, by = C.c_double(), C.c_double()
        self._check(self.lib.fdapde_kron_bench_spmv(self._ctx, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def kron_set_obs(self, Psi, Phi=None, weights=None, scale=-1.0):
        """fdapde_kron_set_obs: the handle's matrix becomes A + scale (Phi (x) Psi)^T W (Phi (x) Psi), the term kept factored.  Psi: a scipy.sparse matrix
        (n_obs x n_dofs; duplicates summed, columns sorted), a triple (rowptr, colidx, values) handed to the library as it is, or None (clears the term).
        Phi: dense p x q, or None ([I_p 0] with p taken from the weights' first axis, else q).  weights: (p, n_obs) or flat (instant-major), or None (W = I)"""
        if Psi is None:
            self._check(self.lib.fdapde_kron_set_obs(self._ctx, 1, None, C.c_int64(0), None, None, None, None, C.c_double(scale)))
            return
        if isinstance(Psi, (tuple, list)):
            rp, ci, v = Psi
        else:
            m = Psi.tocsr().copy()
            m.sum_duplicates()
            m.sort_indices()
            if m.shape[1] != self.sizes()["n_dofs"]:
                raise ValueError("kron_set_obs(): Psi needs n_dofs columns")
            rp, ci, v = m.indptr, m.indices, m.data
        rp = np.ascontiguousarray(rp, dtype=np.int64).reshape(-1)
        ci = np.ascontiguousarray(ci, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(v, dtype=float).reshape(-1)
        if rp.size < 1 or ci.size != v.size or (rp.size > 1 and rp.max() > ci.size):
            raise ValueError("kron_set_obs(): rowptr / colidx / values do not fit together")
        n_obs = rp.size - 1
        phi = None
        if Phi is not None:
            phi = np.asfortranarray(np.asarray(Phi, dtype=float))
            if phi.ndim != 2 or (getattr(self, "_kron_q", 0) and phi.shape[1] != self._kron_q):
                raise ValueError("kron_set_obs(): Phi must be p x q")
            p = phi.shape[0]
        elif weights is not None and np.ndim(weights) == 2:
            p = np.shape(weights)[0]
        elif weights is not None and n_obs > 0:
            p = np.size(weights) // n_obs
        else:
            p = getattr(self, "_kron_q", 0)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=float).reshape(-1)
            if w.size != p * n_obs:
                raise ValueError("kron_set_obs(): p n_obs weights")
        self._check(self.lib.fdapde_kron_set_obs(self._ctx, int(p), None if phi is None else _dp(phi), C.c_int64(n_obs), rp.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 _ip(ci), _dp(v), None if w is None else _dp(w), C.c_double(scale)))

    def kron_obs_info(self):
        """fdapde_kron_obs_info -> dict(p, n_obs, nnz, form_rows, form_cols): the live data term's sizes and the form (1 narrow, 2 wide) for Psi / for Psi^T"""
        p, n_obs, nnz, fr, fc = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        self._check(self.lib.fdapde_kron_obs_info(self._ctx, C.byref(p), C.byref(n_obs), C.byref(nnz), C.byref(fr), C.byref(fc)))
        return {"p": p.value, "n_obs": n_obs.value, "nnz": nnz.value, "form_rows": fr.value, "form_cols": fc.value}

    def kron_amg_hierarchy(self):
        """fdapde_kron_amg_hierarchy: the live hierarchy of FDAPDE_SOLVER_KRON_AMG (rows counted as q n_l, entries as q^2 nnz_l) ->
        dict(rows, nnz: per level, the last level the inverted one; absorbed; setup_ms).  FdapdeError(ENOTINIT) where none is live"""
        nl, ab, ms = C.c_int32(), C.c_int32(), C.c_double()
        self._check(self.lib.fdapde_kron_amg_hierarchy(self._ctx, 0, C.byref(nl), None, None, None, None))
        rows, nnz = np.zeros(nl.value, dtype=np.int64), np.zeros(nl.value, dtype=np.int64)
        self._check(self.lib.fdapde_kron_amg_hierarchy(self._ctx, nl.value, C.byref(nl), rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       nnz.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ab), C.byref(ms)))
        return dict(rows=[int(r) for r in rows], nnz=[int(z) for z in nnz], absorbed=ab.value, setup_ms=ms.value)

    def kron_amg_aggregates(self, level):
        """fdapde_kron_amg_aggregates: for a level of the live hierarchy that has a next one, the DOF of level + 1 every DOF of `level` belongs to (level 0
        in the reference DOF numbering) -> int32 array.  FdapdeError(ENOTINIT) where no hierarchy is live"""
        n = C.c_int64(0)
        rc = self.lib.fdapde_kron_amg_aggregates(self._ctx, int(level), C.c_int64(0), None, C.byref(n))
        if rc != EINVAL or n.value <= 0:   # (a valid level answers EINVAL to the empty buffer and leaves its row count)
            self._check(rc)
        agg = np.full(n.value, -1, dtype=np.int32)
        self._check(self.lib.fdapde_kron_amg_aggregates(self._ctx, int(level), C.c_int64(agg.size), _ip(agg), C.byref(n)))
        return agg

    def gram_pointwise(self, cell_ids, values, weights=None):
        """Psi^T W Psi on the FEM pattern (nnz values aligned with pattern_get()) from cell ids and row-major n_locs x n_basis values"""
        s = self.sizes()
        cells = np.ascontiguousarray(cell_ids, dtype=np.int32).reshape(-1)
        vals = np.ascontiguousarray(values, dtype=float)
        if vals.size != cells.size * s["n_basis"]:
            raise ValueError("gram_pointwise(): values must be n_locs x n_basis")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=float).reshape(-1)
        if w is not None and w.size != cells.size:
            raise ValueError("gram_pointwise(): one weight per location")
        out = np.zeros(s["nnz"])
        self._check(self.lib.fdapde_gram_pointwise(self._ctx, C.c_int64(cells.size), _ip(cells), _dp(vals), None if w is None else _dp(w), _dp(out)))
        return out

    def eval_pointwise_raw(self, locs):
        """fdapde_eval_pointwise as the C ABI hands it out: (cell ids, values n_locs x n_basis)"""
        locs = np.asarray(locs, dtype=float)
        if locs.ndim == 1:
            locs = locs.reshape(-1, 1)
        nl, s = locs.shape[0], self.sizes()
        flat = np.ascontiguousarray(locs.T).reshape(-1)
        cells = np.zeros(nl, dtype=np.int32)
        vals = np.zeros((nl, s["n_basis"]))
        self._check(self.lib.fdapde_eval_pointwise(self._ctx, C.c_int64(nl), _dp(flat), _ip(cells), _dp(vals)))
        return cells, vals

    def project_raw(self, points):
        """fdapde_project as the C ABI hands it out: (cell ids, values n_pts x n_basis, projected points n_pts x N, distances)"""
        pts = np.asarray(points, dtype=float)
        if pts.ndim == 1:
            pts = pts.reshape(-1, 1)
        n, dim, s = pts.shape[0], pts.shape[1], self.sizes()
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        cells = np.zeros(n, dtype=np.int32)
        proj, dist, vals = np.zeros(n * dim), np.zeros(n), np.zeros((n, s["n_basis"]))
        self._check(self.lib.fdapde_project(self._ctx, C.c_int64(n), _dp(flat), _ip(cells), _dp(proj), _dp(dist), _dp(vals)))
        return cells, vals, np.ascontiguousarray(proj.reshape(dim, n).T), dist

    # ---- basis evaluation (PDE__::eval_basis): Psi as scipy CSR + D
    def eval_pointwise(self, locs):
        """pointwise_evaluation::eval -> (Psi csr n_locs x n_dofs, D = ones, cell ids)"""
        import scipy.sparse as sp

        locs = np.asarray(locs, dtype=float)
        if locs.ndim == 1:
            locs = locs.reshape(-1, 1)
        nl, s = locs.shape[0], self.sizes()
        flat = np.ascontiguousarray(locs.T).reshape(-1)
        cells = np.zeros(nl, dtype=np.int32)
        vals = np.zeros((nl, s["n_basis"]))
        self._check(self.lib.fdapde_eval_pointwise(self._ctx, C.c_int64(nl), _dp(flat), _ip(cells), _dp(vals)))
        dofs, _, _ = self.dofs_get()
        ok = cells >= 0
        rows = np.repeat(np.nonzero(ok)[0], s["n_basis"])
        cols = dofs[cells[ok]].reshape(-1)
        psi = sp.csr_matrix((vals[ok].reshape(-1), (rows, cols)), shape=(nl, s["n_dofs"]))
        return psi, np.ones(nl), cells

    def project(self, points, values=True):
        """Projection<Triangulation>(points, Exact) -> (Psi csr n_pts x n_dofs, cell ids, projected points n_pts x N, distances): every point
        onto its nearest cell, Psi the basis at the projected point (None with values=False).  Every row is filled."""
        import scipy.sparse as sp

        pts = np.asarray(points, dtype=float)
        if pts.ndim == 1:
            pts = pts.reshape(-1, 1)
        n, dim, s = pts.shape[0], pts.shape[1], self.sizes()
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        cells = np.zeros(n, dtype=np.int32)
        proj = np.zeros(n * dim)
        dist = np.zeros(n)
        vals = np.zeros((n, s["n_basis"])) if values else None
        self._check(self.lib.fdapde_project(self._ctx, C.c_int64(n), _dp(flat), _ip(cells), _dp(proj), _dp(dist), _dp(vals) if values else None))
        projected = np.ascontiguousarray(proj.reshape(dim, n).T)
        if not values:
            return None, cells, projected, dist
        dofs, _, _ = self.dofs_get()
        rows = np.repeat(np.arange(n), s["n_basis"])
        psi = sp.csr_matrix((vals.reshape(-1), (rows, dofs[cells].reshape(-1))), shape=(n, s["n_dofs"]))
        return psi, cells, projected, dist

    def eval_areal(self, incidence):
        """areal_evaluation::eval: incidence (n_sub, n_cells) of 0/1 -> (Psi csr n_sub x n_dofs, D = subdomain measures)"""
        import scipy.sparse as sp

        inc = sp.csr_matrix(np.asarray(incidence) == 1, dtype=float)
        s = self.sizes()
        meas = np.zeros(self.n_cells)
        pint = np.zeros((self.n_cells, s["n_basis"]))
        self._check(self.lib.fdapde_cell_integrals(self._ctx, _dp(meas), _dp(pint)))
        dofs, _, _ = self.dofs_get()
        D = inc @ meas
        nb = s["n_basis"]
        cellmat = sp.csr_matrix((pint.reshape(-1), (np.repeat(np.arange(self.n_cells), nb), dofs.reshape(-1))),
                                shape=(self.n_cells, s["n_dofs"]))
        psi = sp.diags(1.0 / D) @ (inc @ cellmat)
        return psi.tocsr(), D

    def info(self):
        info = Info()
        self._check(self.lib.fdapde_info_get(self._ctx, C.byref(info)))
        return info

    # ---- getters
    def matrix_values(self, which=MAT_STIFF):
        out = np.zeros(self.sizes()["nnz"])
        self._check(self.lib.fdapde_matrix_values(self._ctx, which, _dp(out)))
        return out

    def lump(self, which=MAT_MASS):
        """diagonal of lump(mass()) / lump(stiff()) (row sums)"""
        out = np.zeros(self.sizes()["n_dofs"])
        self._check(self.lib.fdapde_lump(self._ctx, which, _dp(out)))
        return out

    def force(self, ncols=None):
        """force_ (n_dofs x forcing columns, column after column).  ncols defaults to the columns of the last set_forcing of THIS wrapper: fdapde_force
        writes n_dofs * (forcing columns) doubles whatever the caller expects (a shorter buffer is a heap overrun -- tools/fuzz_handle.py found that
        the hard way)"""
        have = getattr(self, "_force_cols", 1)
        if ncols is None:
            ncols = have
        if ncols < have:
            raise ValueError(f"force(): the context holds {have} forcing columns, a buffer for {ncols} was asked for")
        out = np.zeros(self.sizes()["n_dofs"] * ncols)
        self._check(self.lib.fdapde_force(self._ctx, _dp(out)))
        return out

    def solution(self):
        out = np.zeros(self.sizes()["n_dofs"])
        self._check(self.lib.fdapde_solution(self._ctx, _dp(out)))
        return out

    def spmv(self, which, x):
        x = np.ascontiguousarray(x, dtype=float)
        y = np.zeros_like(x)
        self._check(self.lib.fdapde_spmv(self._ctx, which, _dp(x), _dp(y)))
        return y

    def bench_spmv(self, reps=50):
        ms, by = C.c_double(), C.c_double()
        self._check(self.lib.fdapde_bench_spmv(self._ctx, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def solver_layout(self, with_dirichlet=True):
        """(rows, entries) of the interior block as a plain CSR operator + bytes one in-solve SpMV launch streams"""
        ni, nz, by = C.c_int64(), C.c_int64(), C.c_double()
        self._check(self.lib.fdapde_solver_layout(self._ctx, 1 if with_dirichlet else 0, C.byref(ni), C.byref(nz), C.byref(by)))
        return ni.value, nz.value, by.value

    def solver_layout_kind(self, with_dirichlet=True):
        """dict(kind: 0 CSR | 1 blocked ELL | 2 persistent streaming | 3 persistent resident, sym, workgroups, rows_per_thread)"""
        k, sy, g, r = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.fdapde_solver_layout_kind(self._ctx, 1 if with_dirichlet else 0, C.byref(k), C.byref(sy), C.byref(g), C.byref(r)))
        return dict(kind=k.value, sym=sy.value, workgroups=g.value, rows_per_thread=r.value)

    def solver_layout_partition(self, with_dirichlet=True):
        """0: the single launch's blocks are chunks of the internal order, 1: cut by coordinate bisection, -1: no single-launch layout"""
        p = C.c_int32()
        self._check(self.lib.fdapde_solver_layout_partition(self._ctx, 1 if with_dirichlet else 0, C.byref(p)))
        return p.value

    def solver_trace(self):
        """dict(small_front: the last solve's front ran as k_small_front, graph_replays: chunks of it replayed from a captured graph)"""
        f, g = C.c_int32(), C.c_int32()
        self._check(self.lib.fdapde_solver_trace(self._ctx, C.byref(f), C.byref(g)))
        return dict(small_front=f.value, graph_replays=g.value)

    def solve_reuse_count(self):
        """fdapde_solve calls of this context that took the prepared (Jacobi-scaled, filled) system of the solve before them"""
        n = C.c_int64()
        self._check(self.lib.fdapde_solve_reuse_count(self._ctx, C.byref(n)))
        return n.value

    def amg_hierarchy(self, which=AMG_OF_SOLVE):
        """fdapde_amg_hierarchy: the live hierarchy of fdapde_solve (0), the factor-once handle (1) or the block handle (2, rows counted as 2 n_l) ->
        dict(rows, nnz: per level, the last level the inverted one; absorbed; setup_ms).  FdapdeError(ENOTINIT) where none is live"""
        nl, ab, ms = C.c_int32(), C.c_int32(), C.c_double()
        self._check(self.lib.fdapde_amg_hierarchy(self._ctx, int(which), 0, C.byref(nl), None, None, None, None))
        rows, nnz = np.zeros(nl.value, dtype=np.int64), np.zeros(nl.value, dtype=np.int64)
        self._check(self.lib.fdapde_amg_hierarchy(self._ctx, int(which), nl.value, C.byref(nl), rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  nnz.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ab), C.byref(ms)))
        return dict(rows=[int(r) for r in rows], nnz=[int(z) for z in nnz], absorbed=ab.value, setup_ms=ms.value)

    def amg_cols_trace(self, which):
        """fdapde_amg_cols_trace: since the hierarchy of the factor-once handle (which = 1) or the block handle (2) was built ->
        dict(batches: runs of 2, 4 or 8 columns side by side; batched_cols: the columns they took; single_cols: the columns solved one by one)"""
        b, q, s = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.fdapde_amg_cols_trace(self._ctx, int(which), C.byref(b), C.byref(q), C.byref(s)))
        return dict(batches=b.value, batched_cols=q.value, single_cols=s.value)

    def amg_aggregates(self, which, level):
        """fdapde_amg_aggregates: for a live hierarchy (`which` as amg_hierarchy) and a level that has a next one, the row of level + 1 every row of `level`
        belongs to (the block handle's: block rows; level 0 in the reference DOF numbering; -1: a row of no aggregate, a Dirichlet row of fdapde_solve's level 0)
        -> int32 array.  FdapdeError(ENOTINIT) where no such hierarchy is live"""
        n = C.c_int64(0)
        rc = self.lib.fdapde_amg_aggregates(self._ctx, int(which), int(level), C.c_int64(0), None, C.byref(n))
        if rc != EINVAL or n.value <= 0:   # (a valid level answers EINVAL to the empty buffer and leaves its row count)
            self._check(rc)
        agg = np.full(n.value, -1, dtype=np.int32)
        self._check(self.lib.fdapde_amg_aggregates(self._ctx, int(which), int(level), C.c_int64(agg.size), _ip(agg), C.byref(n)))
        return agg

    def amg_order(self, which):
        """fdapde_amg_order: the reference DOF of every row of a live hierarchy's level 0, in the level's own order -> int32 array"""
        n = C.c_int64(0)
        rc = self.lib.fdapde_amg_order(self._ctx, int(which), C.c_int64(0), None, C.byref(n))
        if rc != EINVAL or n.value <= 0:   # (a live hierarchy answers EINVAL to the empty buffer and leaves its row count)
            self._check(rc)
        order = np.full(n.value, -1, dtype=np.int32)
        self._check(self.lib.fdapde_amg_order(self._ctx, int(which), C.c_int64(order.size), _ip(order), C.byref(n)))
        return order

    def amg_damping(self, which):
        """fdapde_amg_damping: the smoothers' damping of a live hierarchy, per level, exactly as the cycle takes it (0 on the last level, which is inverted;
        the block handle's: 0.7) -> float64 array.  FdapdeError(ENOTINIT) where no such hierarchy is live"""
        nl = C.c_int32()
        self._check(self.lib.fdapde_amg_damping(self._ctx, int(which), 0, C.byref(nl), None))
        om = np.zeros(nl.value, dtype=np.float64)
        self._check(self.lib.fdapde_amg_damping(self._ctx, int(which), nl.value, C.byref(nl), _dp(om)))
        return om

    # ---- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = load().fdapde_comm_unique_id(buf)
        if rc != OK:
            raise FdapdeError(rc, "fdapde_comm_unique_id failed (RCCL not loadable?)")
        return buf.raw

    def comm_init(self, world, rank, unique_id: bytes):
        self._check(self.lib.fdapde_comm_init(self._ctx, int(world), int(rank), C.c_char_p(unique_id)))

    def rowdist_setup(self, dof_key, dof_owner):
        """row-distributed multi-GPU form: global key and owning rank of every local DOF (fdapde_rowdist_setup)"""
        k = np.ascontiguousarray(dof_key, dtype=np.int64)
        o = np.ascontiguousarray(dof_owner, dtype=np.int32)
        self._check(self.lib.fdapde_rowdist_setup(self._ctx, k.ctypes.data_as(C.POINTER(C.c_int64)), _ip(o)))

    def comm_allreduce(self, values, op="sum"):
        """sum / max of a float64 array over the ranks of the communicator (through the library's own RCCL communicator)"""
        a = np.ascontiguousarray(np.asarray(values, dtype=float)).copy()
        self._check(self.lib.fdapde_comm_allreduce(self._ctx, _dp(a), int(a.size), 0 if op == "sum" else 1))
        return a

    def comm_count(self):
        """ranks of the communicator as RCCL reports them (ncclCommCount); the registered world size under the host-staged transport"""
        n = C.c_int32(0)
        self._check(self.lib.fdapde_comm_count(self._ctx, C.byref(n)))
        return int(n.value)

    @staticmethod
    def comm_library():
        return (load().fdapde_comm_library() or b"").decode()

    def comm_init_callback(self, world, rank, allreduce):
        """host-staged transport: allreduce(numpy float64 array) must sum it over all ranks in place"""
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)

        def _cb(user, ptr, count):
            try:
                allreduce(np.ctypeslib.as_array(ptr, shape=(count,)))
                return 0
            except Exception:   # noqa: BLE001  (must not propagate through the C frame)
                return 1

        self._ar_cb = proto(_cb)   # keep alive
        self._check(self.lib.fdapde_comm_init_callback(self._ctx, int(world), int(rank), self._ar_cb, None))

    def halo_setup(self, n_if_global, local_dof, if_index, owned):
        local_dof = np.ascontiguousarray(local_dof, dtype=np.int32)
        if_index = np.ascontiguousarray(if_index, dtype=np.int32)
        owned = np.ascontiguousarray(owned, dtype=np.uint8)
        self._check(self.lib.fdapde_halo_setup(self._ctx, C.c_int64(int(n_if_global)), C.c_int64(local_dof.size), _ip(local_dof),
                                               _ip(if_index), _bp(owned)))

    def comm_set_exchange_callback(self, exchange):
        """host-staged neighbour exchange: exchange(peer_rank (int32 array), peer_off (int64 array), send (float64 array), recv (float64
        array, to fill)) must deliver send[peer_off[q]:peer_off[q + 1]] to rank peer_rank[q] and fill the same segment of recv with
        what that rank sent to this one"""
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double))

        def _cb(user, n_peers, ranks, offs, send, recv):
            try:
                off = np.ctypeslib.as_array(offs, shape=(n_peers + 1,))
                n = int(off[-1])
                exchange(np.ctypeslib.as_array(ranks, shape=(n_peers,)), off, np.ctypeslib.as_array(send, shape=(n,)),
                         np.ctypeslib.as_array(recv, shape=(n,)))
                return 0
            except Exception:   # noqa: BLE001  (must not propagate through the C frame)
                return 1

        self._xchg_cb = proto(_cb)   # keep alive
        self._check(self.lib.fdapde_comm_set_exchange_callback(self._ctx, self._xchg_cb, None))

    def halo_setup_peers(self, peer_rank, peer_off, peer_dof, owned):
        """neighbour-only exchange (fdapde_halo_setup_peers): peer ranks ascending, their segments in peer_dof (DOF ids shared with the
        peer, in an order both ranks of the pair agree on)"""
        peer_rank = np.ascontiguousarray(peer_rank, dtype=np.int32)
        peer_off = np.ascontiguousarray(peer_off, dtype=np.int64)
        peer_dof = np.ascontiguousarray(peer_dof, dtype=np.int32)
        owned = np.ascontiguousarray(owned, dtype=np.uint8)
        self._check(self.lib.fdapde_halo_setup_peers(self._ctx, C.c_int32(peer_rank.size), _ip(peer_rank),
                                                     peer_off.ctypes.data_as(C.POINTER(C.c_int64)), _ip(peer_dof), _bp(owned)))

    def tune(self, key, value):
        self._check(self.lib.fdapde_tune(self._ctx, key.encode(), int(value)))

    def stream(self):
        return self.lib.fdapde_stream(self._ctx)

    def synchronize(self):
        self._check(self.lib.fdapde_synchronize(self._ctx))
