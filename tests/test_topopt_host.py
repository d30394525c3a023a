"""The host surface of element-scaled stiffness and topology optimisation, without a GPU: the new C entry points are
exported, bound and match the header; the scaled operator is the ``ElemOp::Scaled`` instance of the plain element kernels of
``tri3_cg.hip`` / ``quad4_cg.hip`` / ``tri3_amg.hip`` -- 14 + 4 apply instances on the plain apply's dispatch, the diag and
assembly instances, none with scratch, no sibling kernel left -- and ``topopt.hip`` holds the design kernels only; argument
errors come back as negative codes with a message before any device is touched; ``TopologyOptimizer`` refuses what it does not
support; ``set_element_scale(None)`` leaves the solver's sequence of library calls as it was."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ["hfem_cg_setup_scaled", "hfem_amg_assemble_scaled", "hfem_amg_setup_scaled", "hfem_topt_create", "hfem_topt_destroy",
           "hfem_topt_slots", "hfem_topt_weights", "hfem_topt_filter", "hfem_topt_energy", "hfem_topt_oc", "hfem_topt_status"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "hidenn_fem.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1
            for m in re.finditer(r"\bint(?:64_t)?\s+(hfem_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_symbols_are_exported_bound_and_match_the_header():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    counts = _header_arg_counts()
    for n in SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert n in counts, f"{n} is not declared in include/hidenn_fem.h"
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
        assert len(L.PROTOTYPES[n][1]) == counts[n], n
    assert L.lib().hfem_version() == 114


def test_scaled_operator_is_the_scaled_instance_of_the_plain_kernels_without_scratch():
    _lib()
    from hidenn_fem_amd.csrc import build
    assert "topopt.hip" in build.SOURCES
    use = build.resource_usage()
    # no sibling kernels: K(w) is the ElemOp::Scaled instance (the last template argument, value 2) of the plain kernels
    gone = [k for k in use if "scaled_apply_kernel" in k or "scaled_diag_kernel" in k or "amg_assemble_scaled_kernel" in k]
    assert not gone, gone
    scaled = {k: v for k, v in use.items() if re.search(r"L[^L]*6ElemOpE2EE", k)}
    for kernel, count, source in (("tri3_cg_apply_kernel", 14, "tri3_cg.hip"), ("quad4_cg_apply_kernel", 4, "quad4_cg.hip"),
                                  ("tri3_cg_diag_kernel", 4, "tri3_cg.hip"), ("quad4_cg_diag_kernel", 2, "quad4_cg.hip"),
                                  ("amg_assemble_kernel", 4, "tri3_amg.hip")):
        inst = {k: v for k, v in scaled.items() if re.search(r"\d+" + kernel + "I", k)}
        assert len(inst) == count, (kernel, sorted(inst))
        assert all(v["scratch"] == 0 and v["source"] == source for v in inst.values()), (kernel, inst)
    assert len(scaled) == 28, sorted(scaled)
    # the TRI3 apply instances are the plain dispatch's seven tile shapes in both conventions, the QUAD4 ones its two
    shapes = sorted(re.search(r"tri3_cg_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EL", k).groups()
                    for k in scaled if "tri3_cg_apply_kernel" in k)
    want = sorted((b, n, e, p) for b, n, e in (("512", "2", "2"), ("256", "3", "3"), ("256", "3", "4"), ("256", "3", "6"),
                                                ("256", "4", "3"), ("256", "4", "4"), ("256", "4", "6")) for p in "01")
    assert shapes == want
    q = sorted(re.search(r"quad4_cg_apply_kernelILi256ELi(\d)ELi(\d)ELb([01])EL", k).groups()
               for k in scaled if "quad4_cg_apply_kernel" in k)
    assert q == sorted((n, n, p) for n in "34" for p in "01")
    # topopt.hip holds the design handle's kernels and nothing else; none of them lives elsewhere
    mine = {k: v for k, v in use.items() if v["source"] == "topopt.hip"}
    for kernel, count in (("tri3_topt_energy_kernel", 4), ("quad4_topt_energy_kernel", 2), ("topt_weights_kernel", 2),
                          ("topt_filter_kernel", 2), ("topt_oc_init_kernel", 1), ("topt_oc_step_kernel", 2),
                          ("topt_oc_final_kernel", 2)):
        inst = {k: v for k, v in mine.items() if kernel in k}
        assert len(inst) == count, (kernel, sorted(inst))
        assert all(v["scratch"] == 0 for v in inst.values()), (kernel, inst)
    assert all("topt_" in k for k in mine), sorted(k for k in mine if "topt_" not in k)
    assert not [k for k, v in use.items() if "topt_" in k and v["source"] != "topopt.hip"]


def test_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    err = lib.hfem_last_error
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    nan, inf = math.nan, math.inf
    out = C.c_void_p()
    # the scaled setups: the null weights are named; a null handle is a null pointer
    assert lib.hfem_cg_setup_scaled(None, p, None, mat, 0.5, p, 1, None, None) < 0 and b"hfem_cg_setup_scaled: null pointer" in err()
    assert lib.hfem_amg_assemble_scaled(None, p, None, mat, 0.5, p, None) < 0 and b"hfem_amg_assemble_scaled: null pointer" in err()
    assert lib.hfem_amg_setup_scaled(None, p, None, mat, 0.5, p, p, None) < 0 and b"hfem_amg_setup_scaled: null pointer" in err()
    # create
    assert lib.hfem_topt_create(None, p, p, 4, 1.0, C.byref(out)) < 0 and b"hfem_topt_create: null pointer" in err()
    assert lib.hfem_topt_destroy(None) == 0
    assert lib.hfem_topt_slots(None) < 0 and b"hfem_topt_slots: null pointer" in err()
    # weights / energy: the scalars before the handle
    for penal, e_min in ((0.5, 1e-9), (nan, 1e-9), (inf, 1e-9)):
        assert lib.hfem_topt_weights(None, p, penal, e_min, p, p, None) < 0 and b"hfem_topt_weights: penal" in err()
        assert lib.hfem_topt_energy(None, p, None, p, mat, 0.5, 0, p, penal, e_min, p, p, None) < 0
        assert b"hfem_topt_energy: penal" in err()
    for e_min in (-1e-9, 1.0, nan):
        assert lib.hfem_topt_weights(None, p, 3.0, e_min, p, p, None) < 0 and b"hfem_topt_weights: e_min" in err()
        assert lib.hfem_topt_energy(None, p, None, p, mat, 0.5, 0, p, 3.0, e_min, p, p, None) < 0 and b"hfem_topt_energy: e_min" in err()
    assert lib.hfem_topt_energy(None, p, None, p, mat, 0.5, 3, p, 3.0, 1e-9, p, p, None) < 0 and b"hfem_topt_energy: flags" in err()
    assert lib.hfem_topt_weights(None, p, 3.0, 1e-9, p, p, None) < 0 and b"hfem_topt_weights: null pointer" in err()
    assert lib.hfem_topt_energy(None, p, None, p, mat, 0.5, 0, p, 3.0, 1e-9, p, p, None) < 0 and b"hfem_topt_energy: null pointer" in err()
    # filter
    assert lib.hfem_topt_filter(None, p, p + 64, 0, None) < 0 and b"hfem_topt_filter: null pointer" in err()
    # oc: the scalars before the handle
    for vt in (0.0, -1.0, nan, inf):
        assert lib.hfem_topt_oc(None, p, p, p, vt, 0.2, 60, p, p, None) < 0 and b"hfem_topt_oc: vol_target" in err()
    for move in (0.0, -0.1, 1.5, nan):
        assert lib.hfem_topt_oc(None, p, p, p, 1.0, move, 60, p, p, None) < 0 and b"hfem_topt_oc: move" in err()
    for nb in (0, -3, 5000):
        assert lib.hfem_topt_oc(None, p, p, p, 1.0, 0.2, nb, p, p, None) < 0 and b"hfem_topt_oc: n_bisect" in err()
    assert lib.hfem_topt_oc(None, p, p, p, 1.0, 0.2, 60, p, p, None) < 0 and b"hfem_topt_oc: null pointer" in err()
    st = (C.c_double * 16)()
    assert lib.hfem_topt_status(None, st, None) < 0 and b"hfem_topt_status: null pointer" in err()


def test_topt_create_checks_its_plan_and_geometry_without_a_device():
    """A plan created without a device exists on a machine without a GPU: create refuses it, TRI3 and QUAD4, after the checks
    that need no plan."""
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.plan import TilePlan
    lib = _lib().lib()
    out = C.c_void_p()
    for gen, npe in ((structured_tri_mesh, 3), (structured_quad_mesh, 4)):
        nc, conn, geom, bc, mn, edges = gen(9, 7, dtype=torch.float64)
        hp = TilePlan(conn, nc.shape[0], coords_hint=nc, edges=edges, device=None, nodes_per_elem=npe)
        assert lib.hfem_topt_create(hp.handle, None, None, conn.shape[0], 0.0, C.byref(out)) < 0
        assert b"hfem_topt_create: host-only plan" in lib.hfem_last_error() and not out.value
        assert lib.hfem_topt_create(hp.handle, None, None, conn.shape[0], 0.0, None) < 0 and b"null pointer" in lib.hfem_last_error()


def _model(quad=False, dirichlet=True, n=(7, 5), u_fixed=0.0):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    gen, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = gen(*n, dtype=torch.float64)
    return cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc if dirichlet else None, u_fixed=u_fixed, neumann_edges=edges)


def test_topology_optimizer_refuses_what_it_does_not_support():
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D
    from hidenn_fem_amd.topopt import TopologyOptimizer, minimize_compliance_
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="NeoHookeanLoss2D"):
        TopologyOptimizer(_model(), NeoHookeanLoss2D(device=cpu, dtype=torch.float64), 0.4)
    for quad in (False, True):
        with pytest.raises(NotImplementedError, match="deterministic"):
            TopologyOptimizer(_model(quad), EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True), 0.4)
        with pytest.raises(ValueError, match="u_fixed == 0"):
            TopologyOptimizer(_model(quad, u_fixed=0.01), lf, 0.4)
        with pytest.raises(ValueError, match="Dirichlet rows"):
            TopologyOptimizer(_model(quad, dirichlet=False), lf, 0.4, precond="amg")
    for vf in (0.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="volume_fraction"):
            TopologyOptimizer(_model(), lf, vf)
    with pytest.raises(ValueError, match="penal"):
        TopologyOptimizer(_model(), lf, 0.4, penal=0.5)
    for e_min in (0.0, 1.0):
        with pytest.raises(ValueError, match="e_min"):
            TopologyOptimizer(_model(), lf, 0.4, e_min=e_min)
    with pytest.raises(ValueError, match="move"):
        TopologyOptimizer(_model(), lf, 0.4, move=0.0)
    with pytest.raises(ValueError, match="n_bisect"):
        TopologyOptimizer(_model(), lf, 0.4, n_bisect=0)
    with pytest.raises(ValueError, match="filter_radius"):
        TopologyOptimizer(_model(), lf, 0.4, filter_radius=-1.0)
    with pytest.raises(ValueError, match="precond must be"):
        TopologyOptimizer(_model(), lf, 0.4, precond="ilu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TopologyOptimizer(_model(), lf, 0.4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            minimize_compliance_(_model(quad=True), lf, 0.4, precond="block_jacobi")


class _Recorder:
    """Stands in for the loaded library: records the entry points called, returns success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


@pytest.mark.parametrize("quad", [False, True])
def test_set_element_scale_none_leaves_the_call_sequence_as_it_was(quad, monkeypatch):
    """The operator setup of ``refresh`` and the prologue of ``solve`` (up to the first status read; ``max_iter`` 0, so no
    iteration is replayed) on a solver object assembled by hand over a recording library: without a scale the calls are
    today's (``hfem_cg_setup``, the AMG setup; two energy launches, start, status); with one they are the scaled pair, and one
    energy launch plus one standalone apply; and ``set_element_scale(None)`` restores the first lists."""
    from hidenn_fem_amd import _lib as L
    from hidenn_fem_amd import solve as S
    cls = S.Quad4FrozenMeshSolver if quad else S.FrozenMeshSolver
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    monkeypatch.setattr(S, "stream_ptr", lambda dev: None)
    s = cls.__new__(cls)
    z = torch.zeros((3, 2), dtype=torch.float64)
    s._h, s.device, s.precond, s.loss_fn = C.c_void_p(1), torch.device("cpu"), "block_jacobi", type("LF", (), {"_W": 0.5})()
    s._xf, s._xfix, s._ufix, s.diag = z.clone(), z.clone(), z.clone(), torch.zeros((3, 3), dtype=torch.float64)
    s._u, s._zero, s._g0, s._gz, s._loss = z.clone(), z.clone(), z.clone(), z.clone(), torch.zeros((), dtype=torch.float64)
    s._scale, s._graph, s._key = None, None, None
    s.plan = type("P", (), {"handle": C.c_void_p(2)})()
    s._tables = ((C.c_double * 4)(), None, None, None, 0)
    s._status, s.rtol, s.atol, s.max_iter = (C.c_double * 16)(), 1e-8, 0.0, 0
    s.model = type("M", (), {"node_coords_free": z.clone(), "node_coords_fixed": z.clone(), "u_fixed": z.clone(),
                             "u_free": z.clone()})()

    class Amg:
        _h = None

        def setup(self, *a):
            rec.calls.append("amg.setup")

        def setup_scaled(self, *a):
            rec.calls.append("amg.setup_scaled")

    s._amg = Amg()
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)

    def sequence():
        rec.calls.clear()
        s._setup_operator(mat)
        return list(rec.calls)

    energy = "hfem_quad4_energy_plan_ex" if quad else "hfem_tri3_energy_plan"

    def prologue():
        rec.calls.clear()
        s._key = s._state_key()                              # nothing changed since the last refresh
        s.solve()
        return list(rec.calls)

    plain = sequence()
    assert plain == ["hfem_cg_setup", "amg.setup"]
    plain_solve = prologue()
    assert plain_solve == [energy, energy, "hfem_cg_start_amg", "hfem_cg_status"]
    s._scale = type("W", (), {"w_slot": z.clone().view(-1), "w_elem": z.clone().view(-1)})()
    assert sequence() == ["hfem_cg_setup_scaled", "amg.setup_scaled"]
    assert prologue() == [energy, "hfem_cg_apply", "hfem_cg_start_amg", "hfem_cg_status"]
    s._graph = object()
    s.set_element_scale(None)
    assert s._scale is None and s._graph is None and s._key is None
    assert sequence() == plain
    assert prologue() == plain_solve
    # a nonzero Dirichlet value is refused once a scale is set, before the library is called
    s._scale = type("W", (), {"w_slot": z.clone().view(-1), "w_elem": z.clone().view(-1)})()
    s._ufix = torch.full((3, 2), 0.01, dtype=torch.float64)
    rec.calls.clear()
    with pytest.raises(ValueError, match="u_fixed == 0"):
        s._setup_operator(mat)
    assert rec.calls == []


def test_the_product_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys; import hidenn_fem_amd.topopt; assert 'scipy' not in sys.modules, 'scipy imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
