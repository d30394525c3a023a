"""The QUAD4 frozen-mesh solve's host surface, without a GPU: the AMG host setup for 4-node cells (hfem_amg_host_create_ex)
against scipy -- fine pattern, fan, aggregation, symbolic products, repeatability -- its agreement with the TRI3 entry point
for npe = 3, argument errors as codes, and what ``Quad4FrozenMeshSolver`` refuses."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import torch

from test_amg_host import Host, _lib, _row_maps


class HostEx(Host):
    """A host setup through hfem_amg_host_create_ex (npe corners per element)."""

    def __init__(self, conn, x_src, u_src, npe=None):
        self.L = _lib().lib()
        c = np.ascontiguousarray(conn, dtype=np.int32)
        xs, us = np.ascontiguousarray(x_src, dtype=np.int32), np.ascontiguousarray(u_src, dtype=np.int32)
        h = C.c_void_p()
        rc = self.L.hfem_amg_host_create_ex(c.ctypes.data, c.shape[0], c.shape[1] if npe is None else npe, xs.shape[0],
                                            xs.ctypes.data, us.ctypes.data, C.byref(h))
        assert rc == 0, self.L.hfem_last_error()
        self.h = h


def _quad_mesh():
    from hidenn_fem_amd.mesh import structured_quad_mesh
    nc, conn, geom, bc, mn, edges = structured_quad_mesh(61, 41, jitter=0.25)
    assert conn.shape == (60 * 40, 4)
    return conn.numpy().astype(np.int64), bc.numpy().astype(bool), ~geom.numpy().astype(bool)


def _quad_host(order_seed=None):
    conn, bc, xmask = _quad_mesh()
    u_src = _row_maps(~bc, order_seed)
    x_src = _row_maps(xmask, order_seed)
    return HostEx(conn, x_src, u_src), conn, u_src


def _graph(conn, u_src):
    """scipy pattern of the free-node graph of the cells (diagonal + nodes sharing a cell, diagonal partners included)."""
    n = int((u_src >= 0).sum())
    npe = conn.shape[1]
    rows, cols = [np.arange(n)], [np.arange(n)]
    for a in range(npe):
        for b in range(npe):
            ra, rb = u_src[conn[:, a]], u_src[conn[:, b]]
            keep = (ra >= 0) & (rb >= 0)
            rows.append(ra[keep]); cols.append(rb[keep])
    r, c = np.concatenate(rows), np.concatenate(cols)
    g = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    g.sum_duplicates()
    g.sort_indices()
    return g


def test_the_new_symbol_is_exported_and_bound_and_the_version_is_unchanged():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    assert hasattr(h, "hfem_amg_host_create_ex") and "hfem_amg_host_create_ex" in L.PROTOTYPES
    assert L.lib().hfem_amg_host_create_ex.argtypes == L.PROTOTYPES["hfem_amg_host_create_ex"][1]
    assert L.lib().hfem_version() == 114


@pytest.mark.parametrize("order_seed", [None, 5])
def test_quad4_fine_pattern_equals_the_free_node_graph_of_the_cells(order_seed):
    H, conn, u_src = _quad_host(order_seed)
    g = _graph(conn, u_src)
    assert g.getnnz(axis=1).max() == 9                                  # the 9-point graph: diagonal partners are neighbours
    A = H.csr(0, 0, 1, g.shape[1])
    assert A.shape == g.shape
    assert np.array_equal(A.indptr, g.indptr) and np.array_equal(A.indices, g.indices)
    diag = H.arr(0, 2)
    assert np.array_equal(A.indices[diag], np.arange(g.shape[0]))
    top = H.info(-1)
    assert top[1] == g.shape[0] and top[2] == conn.shape[0] and top[5] == 4
    # the fan: every (cell, corner) of a free node once, cell ascending, four slots per record pointing at the right columns
    fp, fe, fc, fs = (H.arr(-1, w) for w in range(4))
    assert fs.shape[0] == 4 * fe.shape[0]
    fs = fs.reshape(-1, 4)
    assert fp[-1] == int((u_src[conn] >= 0).sum()) == top[3]
    for r in range(0, g.shape[0], 37):
        es, cs = fe[fp[r]:fp[r + 1]], fc[fp[r]:fp[r + 1]]
        assert np.all(np.diff(es) > 0)
        assert np.all(u_src[conn[es, cs]] == r)
        for f in range(fp[r], fp[r + 1]):
            for b in range(4):
                c = u_src[conn[fe[f], b]]
                if c < 0:
                    assert fs[f, b] == -1
                else:
                    assert A.indptr[r] <= fs[f, b] < A.indptr[r + 1] and A.indices[fs[f, b]] == c


def test_quad4_aggregates_partition_into_connected_sets_and_repeat_exactly():
    H, conn, u_src = _quad_host(11)
    nlev = H.info(-1)[0]
    assert nlev >= 2
    for lvl in range(nlev - 1):
        n, bs, annz, nagg = H.info(lvl)[:4]
        G = H.csr(lvl, 0, 1, n)
        agg = H.arr(lvl, 3)
        assert agg.shape == (n,) and agg.min() == 0 and agg.max() == nagg - 1 and nagg < n
        assert np.bincount(agg, minlength=nagg).min() >= 1
        order = np.argsort(agg, kind="stable")
        bounds = np.searchsorted(agg[order], np.arange(nagg + 1))
        for a in range(nagg):
            members = order[bounds[a]:bounds[a + 1]]
            ncomp, _ = csgraph.connected_components(G[members][:, members], directed=False)
            assert ncomp == 1, (lvl, a)
        assert H.info(lvl + 1)[0] == nagg and H.info(lvl + 1)[1] == 3
    H2, _, _ = _quad_host(11)
    assert H2.info(-1)[0] == nlev
    for w in range(4):
        assert np.array_equal(H.arr(-1, w), H2.arr(-1, w)), w
    for lvl in range(nlev):
        for w in range(11):
            assert np.array_equal(H.arr(lvl, w), H2.arr(lvl, w)), (lvl, w)


@pytest.mark.parametrize("order_seed", [None, 2])
def test_quad4_symbolic_products_equal_scipys_products_of_the_patterns(order_seed):
    H, conn, u_src = _quad_host(order_seed)
    nlev = H.info(-1)[0]
    assert nlev >= 2
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
        AP = H.csr(lvl, 9, 10, nagg)
        assert same(AP, A @ P) and apnnz == AP.nnz
        assert same(H.csr(lvl + 1, 0, 1, nagg), P.T @ A @ P)


def test_npe3_through_the_new_entry_point_is_the_tri3_hierarchy():
    from hidenn_fem_amd.mesh import structured_tri_mesh
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(61, 41, jitter=0.25, seed=3)
    conn, bc, xmask = conn.numpy().astype(np.int64), bc.numpy().astype(bool), ~geom.numpy().astype(bool)
    u_src, x_src = _row_maps(~bc, 5), _row_maps(xmask, 5)
    H3, Hx = Host(conn, x_src, u_src), HostEx(conn, x_src, u_src, npe=3)
    a, b = H3.info(-1), Hx.info(-1)
    assert a[:4] == b[:4] and a[5] == b[5] == 3
    for w in range(4):
        assert np.array_equal(H3.arr(-1, w), Hx.arr(-1, w)), w
    for lvl in range(a[0]):
        assert H3.info(lvl) == Hx.info(lvl)
        for w in range(11):
            assert np.array_equal(H3.arr(lvl, w), Hx.arr(lvl, w)), (lvl, w)


def test_create_ex_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    out = C.c_void_p()
    src = np.arange(4, dtype=np.int32)
    conn = np.array([[0, 1, 2, 3]], dtype=np.int32)
    for npe in (0, 2, 5, 8):
        assert lib.hfem_amg_host_create_ex(conn.ctypes.data, 1, npe, 4, src.ctypes.data, src.ctypes.data, C.byref(out)) < 0
        assert b"npe" in lib.hfem_last_error()
    assert lib.hfem_amg_host_create_ex(None, 1, 4, 4, src.ctypes.data, src.ctypes.data, C.byref(out)) < 0
    assert b"null pointer" in lib.hfem_last_error()
    assert lib.hfem_amg_host_create_ex(conn.ctypes.data, 1, 4, 4, None, src.ctypes.data, C.byref(out)) < 0
    assert b"null pointer" in lib.hfem_last_error()
    assert lib.hfem_amg_host_create_ex(conn.ctypes.data, 1, 4, 4, src.ctypes.data, src.ctypes.data, None) < 0
    assert b"null pointer" in lib.hfem_last_error()
    bad = np.array([[0, 1, 2, 7]], dtype=np.int32)                     # node 7 does not exist
    assert lib.hfem_amg_host_create_ex(bad.ctypes.data, 1, 4, 4, src.ctypes.data, src.ctypes.data, C.byref(out)) < 0
    assert b"out of range" in lib.hfem_last_error()
    assert lib.hfem_amg_host_create_ex(conn.ctypes.data, 1, 4, 4, src.ctypes.data, src.ctypes.data, C.byref(out)) == 0
    info = (C.c_int64 * 8)()
    try:
        assert lib.hfem_amg_host_info(out, -1, info) == 0 and list(info)[:6][1:4] == [4, 1, 4] and info[5] == 4
    finally:
        lib.hfem_amg_host_destroy(out)


def _model(quad=True):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    mesh = structured_quad_mesh if quad else structured_tri_mesh
    nc, conn, geom, bc, mn, edges = mesh(7, 5, dtype=torch.float64)
    return PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)


def test_quad4_solver_refuses_what_it_does_not_support():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver, solve_displacement_
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="QUAD4"):
        Quad4FrozenMeshSolver(_model(quad=False), lf)
    with pytest.raises(NotImplementedError, match="deterministic"):
        Quad4FrozenMeshSolver(_model(), EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True))
    planless = EnergyLoss2D(device=cpu, dtype=torch.float64)
    planless.quad4_planless = True
    with pytest.raises(NotImplementedError, match="planless"):
        Quad4FrozenMeshSolver(_model(), planless)
    with pytest.raises(ValueError, match="precond"):
        Quad4FrozenMeshSolver(_model(), lf, precond="ilu")
    with pytest.raises(NotImplementedError, match="Quad4FrozenMeshSolver"):     # the TRI3 class names the QUAD4 one
        FrozenMeshSolver(_model(), lf)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Quad4FrozenMeshSolver(_model(), lf)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            solve_displacement_(_model(), lf)


def test_cg_create_on_a_host_only_quad4_plan_reports_host_only():
    from hidenn_fem_amd.mesh import structured_quad_mesh
    from hidenn_fem_amd.plan import TilePlan
    lib = _lib().lib()
    out = C.c_void_p()
    nc, conn, geom, bc, mn, edges = structured_quad_mesh(9, 7, dtype=torch.float64)
    hp = TilePlan(conn, nc.shape[0], coords_hint=nc, edges=edges, device=None, nodes_per_elem=4)
    try:
        assert lib.hfem_cg_create(hp.handle, 10, 0, C.byref(out)) < 0 and b"host-only" in lib.hfem_last_error()
        assert lib.hfem_cg_create(hp.handle, 10, 64, C.byref(out)) < 0 and b"host-only" in lib.hfem_last_error()
    finally:
        hp.close()
