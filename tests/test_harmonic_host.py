"""The harmonic solver's host surface, without a GPU: the new C entry points are exported, bound and match the header, argument
errors come back as negative codes with a message before any device is touched, the new kernels compile without scratch and
beside -- not into -- the instance matrix of the plain apply kernels, and ``HarmonicSolver`` refuses what it does not support."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

HARM_SYMBOLS = ["hfem_harm_create", "hfem_harm_destroy", "hfem_harm_setup", "hfem_harm_apply", "hfem_harm_start",
                "hfem_harm_iterate", "hfem_harm_status"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "hidenn_fem.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(hfem_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_harmonic_symbols_are_exported_bound_and_match_the_header():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    counts = _header_arg_counts()
    for n in HARM_SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert n in counts, f"{n} is not declared in include/hidenn_fem.h"
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
        assert len(L.PROTOTYPES[n][1]) == counts[n], n
    from hidenn_fem_amd.csrc import build
    assert "harmonic.hip" in build.SOURCES
    usage = {k: v for k, v in build.resource_usage().items() if v["source"] == "harmonic.hip"}
    # sibling kernels: the tile shapes of the plain apply's dispatch x PHYS, nothing of them inside tri3_cg.hip / quad4_cg.hip
    for kernel, count in (("tri3_harm_apply_kernel", 14), ("quad4_harm_apply_kernel", 4), ("harm_vec_kernel", 6),
                          ("harm_rz_kernel", 1), ("harm_p_kernel", 1), ("harm_dinv_kernel", 1)):
        inst = {k: v for k, v in usage.items() if kernel in k}
        assert len(inst) == count, (kernel, sorted(inst))
        assert all(v["scratch"] == 0 for v in inst.values()), (kernel, inst)
    assert not [k for k, v in build.resource_usage().items() if "harm" in k and v["source"] != "harmonic.hip"]


def test_harmonic_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    err = lib.hfem_last_error
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    q = p + 256
    nan, inf = math.nan, math.inf
    z = lambda re, im: (C.c_double * 2)(re, im)
    out = C.c_void_p()
    assert lib.hfem_harm_create(None, 10, 0, C.byref(out)) < 0 and b"hfem_harm_create: null pointer" in err()
    assert lib.hfem_harm_destroy(None) == 0
    # setup: the coefficients first (no handle is read), then the handle
    for zk, zm in ((z(0.0, 0.0), z(0.0, 0.0)), (z(nan, 0.0), z(1.0, 0.0)), (z(1.0, inf), z(1.0, 0.0)), (z(1.0, 0.0), z(nan, 0.0)),
                   (z(1.0, 0.0), z(0.0, -inf))):
        assert lib.hfem_harm_setup(None, p, None, mat, 0.5, zk, zm, 0, None) < 0
        assert b"hfem_harm_setup: z_k and z_m must be finite and not all zero" in err()
    assert lib.hfem_harm_setup(None, p, None, mat, 0.5, None, z(1.0, 0.0), 0, None) < 0 and b"null pointer" in err()
    for zk, zm in ((z(1.0, 0.0), z(-4.0, 0.0)), (z(0.0, 1.0), z(0.0, 0.0)), (z(-1.0, -0.5), z(0.0, 2.0))):   # any sign
        assert lib.hfem_harm_setup(None, p, None, mat, 0.5, zk, zm, 0, None) < 0
        assert b"hfem_harm_setup: null pointer" in err()
    # apply / start / iterate: the length (a complex block vector [2][n_u][2]) and the scalars before the handle
    for n in (-4, 1, 2, 3, 6):
        assert lib.hfem_harm_apply(None, p, q, n, p, None) < 0 and b"hfem_harm_apply: len must be a multiple of 4" in err()
        assert lib.hfem_harm_start(None, None, None, p, None, n, 1e-8, 0.0, 10, None) < 0
        assert b"hfem_harm_start: len must be a multiple of 4" in err()
        assert lib.hfem_harm_iterate(None, None, p, n, 1, None) < 0 and b"hfem_harm_iterate: len must be a multiple of 4" in err()
    assert lib.hfem_harm_apply(None, p, q, 8, p, None) < 0 and b"hfem_harm_apply: null pointer" in err()
    for rtol, atol, mi in ((-1.0, 0.0, 10), (1e-8, -1.0, 10), (1e-8, 0.0, -1), (nan, 0.0, 10)):
        assert lib.hfem_harm_start(None, None, None, p, None, 8, rtol, atol, mi, None) < 0
        assert b"hfem_harm_start: rtol, atol and max_iter must be >= 0" in err()
    assert lib.hfem_harm_start(None, None, None, p, None, 8, 1e-8, 0.0, 10, None) < 0 and b"hfem_harm_start: null pointer" in err()
    for n_iter in (0, -1):
        assert lib.hfem_harm_iterate(None, None, p, 8, n_iter, None) < 0 and b"hfem_harm_iterate: n_iter must be > 0" in err()
    assert lib.hfem_harm_iterate(None, None, p, 8, 1, None) < 0 and b"hfem_harm_iterate: null pointer" in err()
    st = (C.c_double * 16)()
    assert lib.hfem_harm_status(None, st, None) < 0 and b"hfem_harm_status: null pointer" in err()


def test_harm_create_refuses_host_only_plans():
    """A plan created without a device exists on a machine without a GPU: create refuses it before it touches a device, TRI3
    and QUAD4, in both conventions; an unknown flag is refused too."""
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.plan import TilePlan
    lib = _lib().lib()
    out = C.c_void_p()
    for gen, npe in ((structured_tri_mesh, 3), (structured_quad_mesh, 4)):
        nc, conn, geom, bc, mn, edges = gen(9, 7, dtype=torch.float64)
        hp = TilePlan(conn, nc.shape[0], coords_hint=nc, edges=edges, device=None, nodes_per_elem=npe)
        for flags in (0, 64):
            assert lib.hfem_harm_create(hp.handle, 10, flags, C.byref(out)) < 0
            assert b"hfem_harm_create: host-only plan" in lib.hfem_last_error() and not out.value
        assert lib.hfem_harm_create(hp.handle, 10, 0, None) < 0 and b"null pointer" in lib.hfem_last_error()


def _model(quad=False, dirichlet=True, n=(7, 5)):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    gen, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = gen(*n, dtype=torch.float64)
    return cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc if dirichlet else None, u_fixed=0.0, neumann_edges=edges)


def test_harmonic_solver_refuses_what_it_does_not_support():
    from hidenn_fem_amd.harmonic import HarmonicSolver, frequency_response
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="NeoHookeanLoss2D"):
        HarmonicSolver(_model(), NeoHookeanLoss2D(device=cpu, dtype=torch.float64))
    for quad in (False, True):
        with pytest.raises(NotImplementedError, match="deterministic"):
            HarmonicSolver(_model(quad), EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True))
        with pytest.raises(ValueError, match="Dirichlet rows"):
            HarmonicSolver(_model(quad, dirichlet=False), lf, precond="amg")
    for ray in ((-1.0, 0.0), (0.0, -1e-3), (math.nan, 0.0), (0.0, math.inf)):
        with pytest.raises(ValueError, match="Rayleigh"):
            HarmonicSolver(_model(), lf, rayleigh=ray)
    for eta in (-0.1, math.nan):
        with pytest.raises(ValueError, match="structural"):
            HarmonicSolver(_model(), lf, structural=eta)
    for rho in (0.0, -2.0):
        with pytest.raises(ValueError, match="density must be > 0"):
            HarmonicSolver(_model(), lf, density=rho)
    with pytest.raises(ValueError, match="mass"):
        HarmonicSolver(_model(), lf, mass="diagonal")
    with pytest.raises(ValueError, match="precond must be"):
        HarmonicSolver(_model(), lf, precond="ilu")
    with pytest.raises(ValueError, match="precond_rebuild"):
        HarmonicSolver(_model(), lf, precond_rebuild="never")
    with pytest.raises(ValueError, match="iters_per_graph"):
        HarmonicSolver(_model(), lf, iters_per_graph=0)
    with pytest.raises(ValueError, match="rtol and atol"):
        HarmonicSolver(_model(), lf, rtol=-1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            HarmonicSolver(_model(), lf)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            HarmonicSolver(_model(quad=True), lf, mass="lumped", precond="block_jacobi")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            frequency_response(_model(quad=True), lf, [0.0, 1.0], precond="none")


def test_the_product_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys; import hidenn_fem_amd.harmonic; assert 'scipy' not in sys.modules, 'scipy imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
