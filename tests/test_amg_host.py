"""Smoothed-aggregation AMG host setup (hidenn_fem_amd/csrc/amg.cpp), without a GPU: the fine block pattern against scipy's
free-node graph, the aggregation (a partition into connected aggregates, no singleton with a neighbour, deterministic), the
symbolic products against scipy's products of the patterns, and argument errors as codes."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

AMG_SYMBOLS = ["hfem_amg_host_create", "hfem_amg_host_destroy", "hfem_amg_host_info", "hfem_amg_host_copy", "hfem_amg_create",
               "hfem_amg_destroy", "hfem_amg_assemble", "hfem_amg_setup", "hfem_amg_set_coarse", "hfem_amg_vcycle",
               "hfem_amg_values", "hfem_cg_start_amg", "hfem_cg_iterate_amg"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def _mesh(kind):
    from hidenn_fem_amd.mesh import structured_tri_mesh, unstructured_tri_mesh
    if kind == "structured":
        nc, conn, geom, bc, mn, edges = structured_tri_mesh(61, 41, jitter=0.25, seed=3)
    else:
        nc, conn, geom, bc, mn, edges = unstructured_tri_mesh(4000)
    return conn.numpy().astype(np.int64), bc.numpy().astype(bool), ~geom.numpy().astype(bool)


def _row_maps(mask, order_seed=None):
    """node -> row map of the nodes of `mask` (rows shuffled when order_seed is given), -1 - k for the others."""
    from hidenn_fem_amd.models import ordered_row_maps
    idx = np.nonzero(mask)[0]
    if order_seed is not None:
        idx = np.random.default_rng(order_seed).permutation(idx)
    return ordered_row_maps(mask, idx)


def _graph(conn, u_src):
    """scipy pattern of the free-node graph (diagonal + nodes sharing an element), over the u rows."""
    n = int((u_src >= 0).sum())
    rows, cols = [np.arange(n)], [np.arange(n)]
    for a in range(3):
        for b in range(3):
            ra, rb = u_src[conn[:, a]], u_src[conn[:, b]]
            keep = (ra >= 0) & (rb >= 0)
            rows.append(ra[keep]); cols.append(rb[keep])
    r, c = np.concatenate(rows), np.concatenate(cols)
    g = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    g.sum_duplicates()
    g.sort_indices()
    return g


class Host:
    def __init__(self, conn, x_src, u_src):
        self.L = _lib().lib()
        c = np.ascontiguousarray(conn, dtype=np.int32)
        xs, us = np.ascontiguousarray(x_src, dtype=np.int32), np.ascontiguousarray(u_src, dtype=np.int32)
        h = C.c_void_p()
        rc = self.L.hfem_amg_host_create(c.ctypes.data, c.shape[0], xs.shape[0], xs.ctypes.data, us.ctypes.data, C.byref(h))
        assert rc == 0, self.L.hfem_last_error()
        self.h = h

    def __del__(self):
        self.L.hfem_amg_host_destroy(self.h)

    def info(self, level):
        out = (C.c_int64 * 8)()
        assert self.L.hfem_amg_host_info(self.h, level, out) == 0
        return list(out)

    def arr(self, level, which):
        n = C.c_int64()
        assert self.L.hfem_amg_host_copy(self.h, level, which, None, C.byref(n)) == 0
        out = np.empty(n.value, dtype=np.int32)
        assert self.L.hfem_amg_host_copy(self.h, level, which, out.ctypes.data, C.byref(n)) == 0
        return out

    def csr(self, level, ptr, col, ncols):
        p, c = self.arr(level, ptr), self.arr(level, col)
        return sp.csr_matrix((np.ones(len(c)), c, p), shape=(len(p) - 1, ncols))


def _host(kind, order_seed=None):
    conn, bc, xmask = _mesh(kind)
    u_src = _row_maps(~bc, order_seed)
    x_src = _row_maps(xmask, order_seed)
    return Host(conn, x_src, u_src), conn, u_src


def test_amg_symbols_are_exported_and_bound():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    for n in AMG_SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
    assert L.lib().hfem_version() == 114


@pytest.mark.parametrize("kind", ["structured", "delaunay"])
@pytest.mark.parametrize("order_seed", [None, 5])
def test_fine_pattern_equals_the_free_node_graph(kind, order_seed):
    H, conn, u_src = _host(kind, order_seed)
    g = _graph(conn, u_src)
    A = H.csr(0, 0, 1, g.shape[1])
    assert A.shape == g.shape
    assert np.array_equal(A.indptr, g.indptr) and np.array_equal(A.indices, g.indices)
    diag = H.arr(0, 2)
    assert np.array_equal(A.indices[diag], np.arange(g.shape[0]))
    # the fan: every (element, corner) of a free node once, element ascending, slots point at the right columns
    fp, fe, fc, fs = (H.arr(-1, w) for w in range(4))
    fs = fs.reshape(-1, 3)
    assert fp[-1] == int((u_src[conn] >= 0).sum())
    for r in range(0, g.shape[0], 37):
        es, cs = fe[fp[r]:fp[r + 1]], fc[fp[r]:fp[r + 1]]
        assert np.all(np.diff(es) > 0)
        assert np.all(u_src[conn[es, cs]] == r)
        for f in range(fp[r], fp[r + 1]):
            for b in range(3):
                c = u_src[conn[fe[f], b]]
                if c < 0:
                    assert fs[f, b] == -1
                else:
                    assert A.indptr[r] <= fs[f, b] < A.indptr[r + 1] and A.indices[fs[f, b]] == c


@pytest.mark.parametrize("kind", ["structured", "delaunay"])
def test_aggregates_partition_into_connected_sets_without_singletons_and_repeat_exactly(kind):
    H, conn, u_src = _host(kind, 11)
    nlev = H.info(-1)[0]
    assert nlev >= 2
    for lvl in range(nlev - 1):
        n, bs, annz, nagg = H.info(lvl)[:4]
        G = H.csr(lvl, 0, 1, n)
        agg = H.arr(lvl, 3)
        assert agg.shape == (n,) and agg.min() == 0 and agg.max() == nagg - 1 and nagg < n
        assert np.bincount(agg, minlength=nagg).min() >= 1          # a partition: every aggregate non-empty, every row in one
        order = np.argsort(agg, kind="stable")
        bounds = np.searchsorted(agg[order], np.arange(nagg + 1))
        for a in range(nagg):
            members = order[bounds[a]:bounds[a + 1]]
            ncomp, _ = csgraph.connected_components(G[members][:, members], directed=False)
            assert ncomp == 1, (lvl, a)
            if len(members) == 1:
                i = members[0]
                assert np.all(G.indices[G.indptr[i]:G.indptr[i + 1]] == i), (lvl, i)   # a singleton has no neighbour
        assert H.info(lvl + 1)[0] == nagg and H.info(lvl + 1)[1] == 3
    n_last, bs_last = H.info(nlev - 1)[:2]
    assert n_last * bs_last <= 1500
    H2, _, _ = _host(kind, 11)
    assert H2.info(-1)[0] == nlev
    for lvl in range(nlev):
        for w in range(11):
            assert np.array_equal(H.arr(lvl, w), H2.arr(lvl, w)), (lvl, w)


@pytest.mark.parametrize("kind", ["structured", "delaunay"])
def test_symbolic_products_equal_scipys_products_of_the_patterns(kind):
    H, conn, u_src = _host(kind, 2)
    nlev = H.info(-1)[0]
    for lvl in range(nlev - 1):
        n, bs, annz, nagg, pnnz, apnnz = H.info(lvl)[:6]
        A = H.csr(lvl, 0, 1, n)
        agg = H.arr(lvl, 3)
        T = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, nagg))
        P = H.csr(lvl, 4, 5, nagg)

        def same(X, Y):
            Y = Y.tocsr()
            Y.sort_indices()
            return np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)

        assert same(P, A @ T) and pnnz == P.nnz
        R = H.csr(lvl, 6, 7, n)
        assert same(R, P.T)
        pidx = H.arr(lvl, 8)                                        # R entry -> its P block
        rows_of_p = np.repeat(np.arange(n), np.diff(P.indptr))
        assert np.array_equal(rows_of_p[pidx], R.indices)
        assert np.array_equal(P.indices[pidx], np.repeat(np.arange(nagg), np.diff(R.indptr)))
        AP = H.csr(lvl, 9, 10, nagg)
        assert same(AP, A @ P) and apnnz == AP.nnz
        assert same(H.csr(lvl + 1, 0, 1, nagg), P.T @ A @ P)


def test_amg_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    out = C.c_void_p()
    assert lib.hfem_amg_host_create(None, 0, 10, None, None, C.byref(out)) < 0 and b"null pointer" in lib.hfem_last_error()
    src = np.arange(3, dtype=np.int32)
    conn = np.array([[0, 1, 5]], dtype=np.int32)                    # node 5 does not exist
    assert lib.hfem_amg_host_create(conn.ctypes.data, 1, 3, src.ctypes.data, src.ctypes.data, C.byref(out)) < 0
    assert b"out of range" in lib.hfem_last_error()
    conn = np.array([[0, 1, 2]], dtype=np.int32)
    bad = np.array([0, 0, 1], dtype=np.int32)                       # two nodes on one row
    assert lib.hfem_amg_host_create(conn.ctypes.data, 1, 3, src.ctypes.data, bad.ctypes.data, C.byref(out)) < 0
    assert b"row map" in lib.hfem_last_error()
    assert lib.hfem_amg_host_destroy(None) == 0 and lib.hfem_amg_destroy(None) == 0
    info = (C.c_int64 * 8)()
    n = C.c_int64()
    assert lib.hfem_amg_host_info(None, 0, info) < 0
    assert lib.hfem_amg_host_copy(None, 0, 0, None, C.byref(n)) < 0
    assert lib.hfem_amg_create(0, None, 0, C.byref(out)) < 0 and b"null pointer" in lib.hfem_last_error()
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    assert lib.hfem_amg_setup(None, None, None, mat, 0.5, None, None) < 0
    assert lib.hfem_amg_assemble(None, None, None, mat, 0.5, None) < 0
    assert lib.hfem_amg_set_coarse(None, None) < 0
    assert lib.hfem_amg_vcycle(None, None, None, None) < 0
    assert lib.hfem_amg_values(None, 0, 0, None, C.byref(n), None) < 0
    assert lib.hfem_cg_start_amg(None, None, None, None, 1e-8, 0.0, 10, None) < 0
    assert lib.hfem_cg_iterate_amg(None, None, None, 1, None) < 0
    # a valid host; bad level / which
    conn = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    us = np.array([-1, 0, 1, 2], dtype=np.int32)
    xs = np.arange(4, dtype=np.int32)
    assert lib.hfem_amg_host_create(conn.ctypes.data, 2, 4, xs.ctypes.data, us.ctypes.data, C.byref(out)) == 0
    try:
        assert lib.hfem_amg_host_info(out, 5, info) < 0 and b"level" in lib.hfem_last_error()
        assert lib.hfem_amg_host_copy(out, 0, 99, None, C.byref(n)) < 0 and b"which" in lib.hfem_last_error()
        assert lib.hfem_amg_host_info(out, -1, info) == 0 and info[0] == 1 and info[1] == 3
    finally:
        lib.hfem_amg_host_destroy(out)


def test_solver_refuses_amg_without_dirichlet_rows_and_unknown_preconditioners():
    import torch
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.solve import FrozenMeshSolver
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(11, 7, dtype=torch.float64)
    lf = EnergyLoss2D(dtype=torch.float64)
    free = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=None, u_fixed=None, neumann_edges=edges)
    with pytest.raises(ValueError, match="Dirichlet"):
        FrozenMeshSolver(free, lf, precond="amg")
    held = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)
    with pytest.raises(ValueError, match="precond"):
        FrozenMeshSolver(held, lf, precond="multigrid")
