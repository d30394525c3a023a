"""The frozen-mesh solve's host surface, without a GPU: the C entry points are exported and bound, argument errors come back
as negative codes with a message before any device is touched, and the Python API refuses what it does not support."""
import ctypes as C

import pytest
import torch

CG_SYMBOLS = ["hfem_cg_create", "hfem_cg_destroy", "hfem_cg_setup", "hfem_cg_start", "hfem_cg_iterate", "hfem_cg_status",
              "hfem_cg_apply"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def test_cg_symbols_are_exported_and_bound_and_the_version_is_unchanged():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    for n in CG_SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
    assert L.lib().hfem_version() == 114


def test_cg_argument_errors_are_negative_codes_with_messages():
    L = _lib()
    lib = L.lib()
    out = C.c_void_p()
    assert lib.hfem_cg_create(None, 10, 0, C.byref(out)) < 0 and b"null pointer" in lib.hfem_last_error()
    assert lib.hfem_cg_destroy(None) == 0
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    assert lib.hfem_cg_setup(None, None, None, mat, 0.5, 1, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
    assert lib.hfem_cg_start(None, None, None, 1e-8, 0.0, 10, None) < 0
    assert lib.hfem_cg_iterate(None, None, 1, None) < 0
    st = (C.c_double * 16)()
    assert lib.hfem_cg_status(None, st, None) < 0
    assert lib.hfem_cg_apply(None, None, None, None, None) < 0 and b"hfem_cg_apply" in lib.hfem_last_error()
    # a host-only plan (device < 0) cannot launch: refused before any device is touched
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.plan import TilePlan
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(9, 7, dtype=torch.float64)
    hp = TilePlan(conn, nc.shape[0], coords_hint=nc, edges=edges, device=None)
    try:
        assert lib.hfem_cg_create(hp.handle, 10, 0, C.byref(out)) < 0 and b"host-only" in lib.hfem_last_error()
        assert lib.hfem_cg_create(hp.handle, 10, 1, C.byref(out)) < 0
    finally:
        hp.close()


def _tri_model(quad=False):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    if quad:
        nc, conn, geom, bc, mn, edges = structured_quad_mesh(7, 5, dtype=torch.float64)
        return QuadShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(7, 5, dtype=torch.float64)
    return PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)


def test_solver_refuses_what_it_does_not_support():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import FrozenMeshSolver, solve_displacement_
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="TRI3"):
        FrozenMeshSolver(_tri_model(quad=True), lf)
    with pytest.raises(NotImplementedError, match="deterministic"):
        FrozenMeshSolver(_tri_model(), EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True))
    with pytest.raises(ValueError):
        FrozenMeshSolver(_tri_model(), lf, precond="ilu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FrozenMeshSolver(_tri_model(), lf)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            solve_displacement_(_tri_model(), lf)
