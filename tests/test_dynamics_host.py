"""The transient-dynamics solver's host surface, without a GPU: the new C entry points are exported, bound and match the header,
argument errors come back as negative codes with a message before any device is touched, and ``NewmarkSolver`` refuses what it
does not support."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

DYN_SYMBOLS = ["hfem_cg_setup_shifted", "hfem_amg_assemble_shifted", "hfem_amg_setup_shifted", "hfem_newmark_predict",
               "hfem_newmark_rhs", "hfem_newmark_correct"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "hidenn_fem.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(hfem_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_dynamics_symbols_are_exported_bound_and_match_the_header():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    counts = _header_arg_counts()
    for n in DYN_SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert n in counts, f"{n} is not declared in include/hidenn_fem.h"
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
        assert len(L.PROTOTYPES[n][1]) == counts[n], n
    from hidenn_fem_amd.csrc import build
    assert "dynamics.hip" in build.SOURCES
    assert not [s for s in build.SOURCES if s.endswith("_dyn_cg.hip")]
    usage = build.resource_usage()
    # The shifted operator is the Mass instance of the plain kernels: the last template argument is the operator tag ElemOp
    # { Plain, Mass, Scaled } (L..6ElemOpE0E | 1E | 2E in the mangled name).  One instance matrix, compiled for each of the three:
    # TRI3 apply (512,2,2) and (256, 3|4, 3|4|6) x PHYS, TRI3 diag (512,2,2), (256,4,6) x PHYS; QUAD4 apply (256,3,3), (256,4,4) x
    # PHYS, QUAD4 diag (256,4,4) x PHYS; assembly 3|4 x PHYS.
    for kernel, count in (("tri3_cg_apply_kernel", 14), ("tri3_cg_diag_kernel", 4), ("quad4_cg_apply_kernel", 4),
                          ("quad4_cg_diag_kernel", 2), ("amg_assemble_kernel", 4)):
        by_op = {"0": {}, "1": {}, "2": {}}
        for name, v in usage.items():
            m = re.search(r"\d+" + kernel + r"I((?:L[ib]\d+E)+)(.*?)EEv", name)   # ...E of the template list, E of the name
            if m:
                tag = re.fullmatch(r"L[^L]*6ElemOpE(\d)E", m.group(2))
                assert tag, f"{name}: the last template argument is not the operator tag ElemOp"
                by_op[tag.group(1)][name] = v
        for op, inst in by_op.items():
            assert len(inst) == count, (kernel, op, sorted(inst))
            assert all(v["scratch"] == 0 for v in inst.values()), (kernel, op, inst)
    for kernel in ("newmark_predict_kernel", "newmark_rhs_kernel", "newmark_correct_kernel"):
        inst = {k: v for k, v in usage.items() if kernel in k}
        assert inst, kernel
        assert all(v["scratch"] == 0 for v in inst.values()), (kernel, inst)


def test_dynamics_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    err = lib.hfem_last_error
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    nan, inf = math.nan, math.inf
    # the shifted setups: coefficients first (no handle is read), then the handles
    for c_k, c_m in ((0.0, 0.0), (-1.0, 1.0), (1.0, -1.0), (nan, 1.0), (1.0, inf)):
        assert lib.hfem_cg_setup_shifted(None, p, None, mat, 0.5, c_k, c_m, 0, 1, None, None) < 0
        assert b"hfem_cg_setup_shifted: c_k and c_m" in err()
        assert lib.hfem_amg_assemble_shifted(None, p, None, mat, 0.5, c_k, c_m, 0, None) < 0
        assert b"hfem_amg_assemble_shifted: c_k and c_m" in err()
        assert lib.hfem_amg_setup_shifted(None, p, None, mat, 0.5, c_k, c_m, 0, p, None) < 0
        assert b"hfem_amg_setup_shifted: c_k and c_m" in err()
    assert lib.hfem_cg_setup_shifted(None, p, None, mat, 0.5, 1.0, 1.0, 0, 1, None, None) < 0
    assert b"hfem_cg_setup_shifted: null pointer" in err()
    assert lib.hfem_amg_assemble_shifted(None, p, None, mat, 0.5, 1.0, 1.0, 0, None) < 0
    assert b"hfem_amg_assemble_shifted: null pointer" in err()
    assert lib.hfem_amg_setup_shifted(None, p, None, mat, 0.5, 0.0, 1.0, 1, p, None) < 0
    assert b"hfem_amg_setup_shifted: null pointer" in err()
    # the vector kernels
    u, v, a, o0, o1, o2 = (p + 64 * i for i in range(6))
    pred = lambda device=0, u=u, n=2, dt=0.1, o0=o0, o2=o2: lib.hfem_newmark_predict(device, u, v, a, n, dt, 0.25, 0.5, 0.0, o0,
                                                                                      o1, o2, None)
    assert pred(device=-1) < 0 and b"hfem_newmark_predict: negative device" in err()
    assert pred(u=None) < 0 and b"hfem_newmark_predict: null pointer" in err()
    assert pred(n=3) < 0 and b"even" in err()
    assert pred(n=-2) < 0 and b"even" in err()
    assert pred(dt=nan) < 0 and b"non-finite" in err()
    assert pred(o0=u) < 0 and b"must differ" in err()
    assert pred(o2=o1) < 0 and b"must differ" in err()
    assert pred(n=0) == 0                                     # nothing to do: no device is touched
    rhs = lambda device=0, b0=u, mv=a, n=2, load=1.0, g0=o0, gz=o1: lib.hfem_newmark_rhs(device, b0, v, mv, o2, n, load, 0.1, g0,
                                                                                          gz, None)
    assert rhs(device=-1) < 0 and b"hfem_newmark_rhs: negative device" in err()
    assert rhs(b0=None) < 0 and b"hfem_newmark_rhs: null pointer" in err()
    assert rhs(n=5) < 0 and b"even" in err()
    assert rhs(load=inf) < 0 and b"non-finite" in err()
    assert rhs(g0=o1) < 0 and b"must differ" in err()
    assert rhs(gz=u) < 0 and b"must differ" in err()
    assert rhs(n=0, mv=None) == 0
    cor = lambda device=0, ut=u, n=2, dt=0.1, uo=o0, vo=o1: lib.hfem_newmark_correct(device, ut, v, a, n, dt, 0.25, 0.5, uo, vo, None)
    assert cor(device=-1) < 0 and b"hfem_newmark_correct: negative device" in err()
    assert cor(ut=None) < 0 and b"hfem_newmark_correct: null pointer" in err()
    assert cor(n=1) < 0 and b"even" in err()
    assert cor(dt=nan) < 0 and b"non-finite" in err()
    assert cor(uo=a) < 0 and b"alias" in err()
    assert cor(uo=v) < 0 and b"alias" in err()
    assert cor(n=0, uo=u, vo=v) == 0                          # in place is allowed


def _model(quad=False, dirichlet=True, n=(7, 5)):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    gen, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = gen(*n, dtype=torch.float64)
    return cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc if dirichlet else None, u_fixed=0.0, neumann_edges=edges)


def test_newmark_solver_refuses_what_it_does_not_support():
    from hidenn_fem_amd.dynamics import NewmarkSolver, transient_
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="NeoHookeanLoss2D"):
        NewmarkSolver(_model(), NeoHookeanLoss2D(device=cpu, dtype=torch.float64), 0.1)
    for quad in (False, True):
        with pytest.raises(NotImplementedError, match="deterministic"):
            NewmarkSolver(_model(quad), EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True), 0.1)
        with pytest.raises(ValueError, match="Dirichlet rows"):
            NewmarkSolver(_model(quad, dirichlet=False), lf, 0.1, precond="amg")
    for dt in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="dt must be > 0"):
            NewmarkSolver(_model(), lf, dt)
    with pytest.raises(ValueError, match="beta must be >= 0"):
        NewmarkSolver(_model(), lf, 0.1, beta=-0.1)
    with pytest.raises(ValueError, match="gamma must be >= 1/2"):
        NewmarkSolver(_model(), lf, 0.1, gamma=0.4)
    for ray in ((-1.0, 0.0), (0.0, -1e-3)):
        with pytest.raises(ValueError, match="Rayleigh"):
            NewmarkSolver(_model(), lf, 0.1, rayleigh=ray)
    for rho in (0.0, -2.0):
        with pytest.raises(ValueError, match="density must be > 0"):
            NewmarkSolver(_model(), lf, 0.1, density=rho)
    with pytest.raises(ValueError, match="c_K"):
        NewmarkSolver(_model(), lf, 0.1, beta=0.0, precond="amg")                 # explicit: A is a pure mass matrix
    with pytest.raises(ValueError, match="mass"):
        NewmarkSolver(_model(), lf, 0.1, mass="diagonal")
    with pytest.raises(ValueError, match="precond"):
        NewmarkSolver(_model(), lf, 0.1, precond="ilu")
    with pytest.raises(ValueError, match="iters_per_graph"):
        NewmarkSolver(_model(), lf, 0.1, iters_per_graph=0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            NewmarkSolver(_model(), lf, 0.1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            NewmarkSolver(_model(quad=True), lf, 0.1, beta=0.0, mass="lumped", precond="block_jacobi")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            transient_(_model(quad=True), lf, 2, 0.1, precond="none")


def test_the_product_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys; import hidenn_fem_amd.dynamics; assert 'scipy' not in sys.modules, 'scipy imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
