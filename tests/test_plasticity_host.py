"""J2 elastoplasticity without a GPU: the new symbols are exported and bound, argument errors are reported before a device is
touched, every refusal the loss and the solvers promise, and the new kernels live outside the existing .hip files."""
import ctypes as C
import os

import pytest
import torch

from conftest import ROOT

SYMBOLS = ["hfem_j2_create", "hfem_j2_destroy", "hfem_j2_slots", "hfem_j2_update", "hfem_j2_commit", "hfem_j2_get", "hfem_j2_set",
           "hfem_cg_setup_j2"]
CSRC = os.path.join(ROOT, "hidenn_fem_amd", "csrc")


def test_symbols_are_exported_and_bound_and_the_version_stays():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    h = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "hidenn_fem.h")).read()
    for n in SYMBOLS:
        assert hasattr(h, n) and n in _lib.PROTOTYPES and n + "(" in header
    assert _lib.lib().hfem_version() == 114
    # append-only header: the J2 block comes after everything that was there
    assert header.index("hfem_j2_create(") > header.index("int hfem_topt_status(")
    assert "tri3_j2.hip" in build.SOURCES and "hfem_j2_dev.h" in build.HEADERS


def test_argument_errors_are_reported_without_a_device():
    from hidenn_fem_amd import _lib
    L = _lib.lib()
    out = C.c_void_p()
    mat = (C.c_double * 4)(1.0, 1.0, 1.0, 0.0)
    assert L.hfem_j2_create(None, 10, mat, 0.5, C.byref(out)) < 0 and b"null pointer" in L.hfem_last_error()
    assert L.hfem_j2_slots(None) < 0
    assert L.hfem_j2_update(None, None, None, None, None, None, 1.0, 0, None, None, None) < 0
    assert L.hfem_j2_commit(None, None) < 0 and L.hfem_j2_get(None, 0, None, None) < 0 and L.hfem_j2_set(None, None, None) < 0
    assert L.hfem_cg_setup_j2(None, None, None, None, None, None, None, 1, None, None, None) < 0
    assert b"null pointer" in L.hfem_last_error()
    assert L.hfem_j2_destroy(None) == 0
    # a host-only plan: refused before any device call; so are a paired plan's slots and bad material constants
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.plan import TilePlan
    coords, conn = structured_tri_mesh(6, 5, dtype=torch.float64)[:2]
    plan = TilePlan(conn, coords.shape[0], coords_hint=coords, device=None, elem_order=3, nodes_per_elem=3)
    assert L.hfem_j2_create(plan.handle, conn.shape[0], mat, 0.5, C.byref(out)) < 0 and b"host-only" in L.hfem_last_error()
    assert not out.value


def loss(**kw):
    from hidenn_fem_amd.plasticity import J2PlasticityLoss2D
    kw.setdefault("device", torch.device("cpu"))
    kw.setdefault("dtype", torch.float64)
    return J2PlasticityLoss2D(**kw)


def test_the_loss_describes_the_material_and_refuses_what_it_cannot_do():
    lf = loss(E=10e9, nu=0.3, sigma_y=6e4, hardening=5e8)
    mu, lam = 10e9 / 2.6, 10e9 * 0.3 / (1.3 * 0.4)
    assert lf.grad_convention == "physical" and lf.plane == "strain"
    assert abs(lf.lame[0] - lam) <= 1e-6 * lam and abs(lf.lame[1] - mu) <= 1e-6 * mu
    assert abs(lf.kappa - (lam + 2 * mu / 3)) <= 1e-6 * lam and lf.sigma_y == 6e4 and lf.hardening == 5e8
    assert len(lf._body_table(None)) == 6                                  # the force tables are EnergyLoss2D's
    for bad in (dict(sigma_y=0.0), dict(sigma_y=-1.0), dict(hardening=-1.0), dict(sigma_y=float("nan"))):
        with pytest.raises(ValueError):
            loss(**bad)
    with pytest.raises(NotImplementedError):
        loss(deterministic=True)
    with pytest.raises(NotImplementedError):
        loss(arithmetic="fp32")
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, _, edges = structured_tri_mesh(6, 5)
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)
    for call in (lambda: lf(m), lambda: lf.domain_energy(m), lambda: lf.value_and_grad_(m)):
        with pytest.raises(NotImplementedError, match="ElastoplasticSolver"):
            call()


def test_every_other_solver_refuses_the_loss():
    from hidenn_fem_amd.loss import EnergyLoss2D, require_linear
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver, assemble_tangent
    from hidenn_fem_amd.plasticity import ElastoplasticSolver
    lf = loss()
    for who in ("FrozenMeshSolver", "NewmarkSolver", "ModalSolver", "TopologyOptimizer", "HarmonicSolver", "StressRecovery"):
        with pytest.raises(NotImplementedError, match="ElastoplasticSolver") as e:
            require_linear(lf, who)
        assert who in str(e.value)
    require_linear(EnergyLoss2D(device=torch.device("cpu")), "FrozenMeshSolver")       # unchanged for a linear loss
    nc, conn, geom, bc, _, edges = structured_tri_mesh(6, 5, dtype=torch.float64)
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)
    q = structured_quad_mesh(5, 4, dtype=torch.float64)
    quad = PiecewiseLinearShapeNN2D(q[0], q[1])
    for check in (NewtonKrylovSolver._check_model, Quad4NewtonKrylovSolver._check_model):
        with pytest.raises(NotImplementedError):
            check(m, lf)
    with pytest.raises(NotImplementedError):
        assemble_tangent(m, lf)
    # the r-adaptive, modal, dynamic and design solvers refuse it in their constructors, before any device work
    from hidenn_fem_amd.dynamics import HyperNewmarkSolver, NewmarkSolver
    from hidenn_fem_amd.modal import ModalSolver
    from hidenn_fem_amd.radapt import HyperRAdaptiveSolver, RAdaptiveSolver
    from hidenn_fem_amd.topopt import TopologyOptimizer
    for build in (lambda: NewmarkSolver(m, lf, 1e-3), lambda: HyperNewmarkSolver(m, lf, 1e-3), lambda: ModalSolver(m, lf),
                  lambda: TopologyOptimizer(m, lf, 0.4), lambda: RAdaptiveSolver(m, lf), lambda: HyperRAdaptiveSolver(m, lf)):
        with pytest.raises(NotImplementedError):
            build()
    # the solver's own checks: the loss kind, QUAD4 models, the preconditioner
    with pytest.raises(NotImplementedError):
        ElastoplasticSolver._check_model(m, EnergyLoss2D(device=torch.device("cpu")))
    with pytest.raises(NotImplementedError, match="TRI3"):
        ElastoplasticSolver._check_model(quad, lf)
    ElastoplasticSolver._check_model(m, lf)
    with pytest.raises(ValueError):
        ElastoplasticSolver(m, lf, precond="amg_tangent")


def test_the_new_kernels_live_outside_the_existing_hip_files():
    names = ["tri3_j2_update_kernel", "tri3_j2_diag_kernel", "tri3_j2_apply_kernel", "j2_finish_kernel", "j2_info_kernel"]
    own = open(os.path.join(CSRC, "tri3_j2.hip")).read()
    for n in names:
        assert n in own
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip") and f != "tri3_j2.hip":
            text = open(os.path.join(CSRC, f)).read()
            assert "__global__" not in text or not any(n in text for n in names), f
            assert "j2_return_map" not in text and "j2_tangent_apply" not in text, f
    from hidenn_fem_amd.csrc import build
    build.build()
    use = build.resource_usage()
    mine = {k: v for k, v in use.items() if v["source"] == "tri3_j2.hip"}
    assert len(mine) == 5 and all(v["scratch"] == 0 for v in mine.values())
    assert not [k for k, v in use.items() if any(n in k for n in names) and v["source"] != "tri3_j2.hip"]
