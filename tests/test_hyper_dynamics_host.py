"""The finite-strain transient solver's host surface, without a GPU: the new C entry points are exported, bound and match the
header, the tangent kernels exist without and with the mass and use no scratch, argument errors come back as negative codes
with a message before any device is touched, and ``HyperNewmarkSolver`` refuses what it does not support."""
import ctypes as C
import math
import re

import pytest
import torch

from test_dynamics_host import _header_arg_counts, _lib, _model

SYMBOLS = ["hfem_cg_setup_hyper_shifted", "hfem_newmark_trial", "hfem_newmark_residual"]


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


def test_tangent_kernels_have_a_plain_and_a_mass_instance_without_scratch():
    """The last template argument (Lb0E | Lb1E in the mangled name) is the bool MASS; one instance each way per kernel."""
    _lib()
    from hidenn_fem_amd.csrc import build
    usage = build.resource_usage()
    for kernel in ("tri3_hyper_cg_apply_kernel", "tri3_hyper_cg_diag_kernel", "quad4_hyper_cg_apply_kernel",
                   "quad4_hyper_cg_diag_kernel"):
        by_mass = {False: [], True: []}
        for name, v in usage.items():
            m = re.search(r"\d+" + kernel + r"I((?:L[ib]\d+E)+)E", name)
            if m:
                last = re.findall(r"L([ib])(\d+)E", m.group(1))[-1]
                assert last[0] == "b", f"{name}: the last template argument is not the bool MASS"
                by_mass[last[1] == "1"].append(v)
        for mass, inst in by_mass.items():
            assert len(inst) == 1, (kernel, mass, inst)
            assert inst[0]["scratch"] == 0, (kernel, mass, inst)
    for kernel in ("newmark_trial_kernel", "newmark_residual_kernel"):
        inst = {k: v for k, v in usage.items() if kernel in k}
        assert inst and all(v["scratch"] == 0 for v in inst.values()), (kernel, inst)


def test_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    err = lib.hfem_last_error
    lame = (C.c_double * 2)(1.0, 0.4)
    buf = (C.c_double * 96)()
    p = C.addressof(buf)
    nan, inf = math.nan, math.inf
    # coefficients first (no handle is read), then the handle
    for c_k, c_m in ((0.0, 0.0), (-1.0, 1.0), (1.0, -1.0), (nan, 1.0), (1.0, inf)):
        assert lib.hfem_cg_setup_hyper_shifted(None, p, None, p, None, lame, 0.5, c_k, c_m, 0, 1, None, None, None) < 0
        assert b"hfem_cg_setup_hyper_shifted: c_k and c_m" in err()
    assert lib.hfem_cg_setup_hyper_shifted(None, p, None, p, None, lame, 0.5, 0.0, 1.0, 0, 1, None, None, None) < 0
    assert b"null pointer" in err()
    a, d, ut, ma, md, o0, o1, o2 = (p + 64 * i for i in range(8))
    tr = lambda device=0, a=a, n=2, s=0.5, c_k=0.1, o0=o0, o1=o1, o2=o2: lib.hfem_newmark_trial(device, a, d, ut, ma, md, n, s, c_k,
                                                                                                o0, o1, o2, None)
    assert tr(device=-1) < 0 and b"hfem_newmark_trial: negative device" in err()
    assert tr(a=None) < 0 and b"hfem_newmark_trial: null pointer" in err()
    assert tr(n=3) < 0 and b"even" in err()
    assert tr(s=nan) < 0 and b"non-finite" in err()
    assert tr(c_k=inf) < 0 and b"non-finite" in err()
    assert tr(o1=o0) < 0 and b"alias" in err()
    assert tr(o1=ut) < 0 and b"alias" in err()
    assert tr(o0=d) < 0 and b"alias" in err()
    assert tr(n=0, o0=a, o2=ma) == 0                          # in place on a and M a is allowed; nothing to do: no device
    rs = lambda device=0, ma=ma, mv=md, n=2, load=1.0, r=o0, neg=o1: lib.hfem_newmark_residual(device, ma, mv, ut, d, n, 1.0, 0.1,
                                                                                                load, r, neg, None)
    assert rs(device=-1) < 0 and b"hfem_newmark_residual: negative device" in err()
    assert rs(ma=None) < 0 and b"hfem_newmark_residual: null pointer" in err()
    assert rs(r=None) < 0 and b"hfem_newmark_residual: null pointer" in err()
    assert rs(n=5) < 0 and b"even" in err()
    assert rs(load=nan) < 0 and b"non-finite" in err()
    assert rs(neg=o0) < 0 and b"must differ" in err()
    assert rs(r=ut) < 0 and b"must differ" in err()
    assert rs(neg=d) < 0 and b"must differ" in err()
    assert rs(n=0, mv=None, neg=None) == 0


def test_hyper_newmark_solver_refuses_what_it_does_not_support():
    from hidenn_fem_amd.dynamics import HyperNewmarkSolver, NewmarkSolver, hyper_transient_
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    cpu = torch.device("cpu")
    lf = NeoHookeanLoss2D(device=cpu, dtype=torch.float64)
    lq = Quad4NeoHookeanLoss2D(device=cpu, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="NewmarkSolver"):
        HyperNewmarkSolver(_model(), EnergyLoss2D(device=cpu, dtype=torch.float64), 0.1)
    with pytest.raises(NotImplementedError, match="Quad4NeoHookeanLoss2D"):
        HyperNewmarkSolver(_model(quad=True), lf, 0.1)                          # QUAD4 model, TRI3 loss
    with pytest.raises(NotImplementedError, match="Quad4NeoHookeanLoss2D"):
        HyperNewmarkSolver(_model(), lq, 0.1)                                   # TRI3 model, QUAD4 loss
    with pytest.raises(NotImplementedError, match="NeoHookeanLoss2D"):          # unchanged: the linear solver still refuses
        NewmarkSolver(_model(), lf, 0.1)
    for quad, loss in ((False, lf), (True, lq)):
        m = lambda **kw: _model(quad, **kw)
        for ray in ((0.0, 1e-3), (0.1, 0.5)):
            with pytest.raises(ValueError, match="mass-proportional"):
                HyperNewmarkSolver(m(), loss, 0.1, rayleigh=ray)
        with pytest.raises(ValueError, match="Rayleigh"):
            HyperNewmarkSolver(m(), loss, 0.1, rayleigh=(-1.0, 0.0))
        with pytest.raises(ValueError, match="Dirichlet rows"):
            HyperNewmarkSolver(m(dirichlet=False), loss, 0.1, precond="amg")
        with pytest.raises(ValueError, match="c_K"):
            HyperNewmarkSolver(m(), loss, 0.1, beta=0.0, precond="amg")
        for dt in (0.0, -1.0, math.nan):
            with pytest.raises(ValueError, match="dt must be > 0"):
                HyperNewmarkSolver(m(), loss, dt)
        with pytest.raises(ValueError, match="beta must be >= 0"):
            HyperNewmarkSolver(m(), loss, 0.1, beta=-0.1)
        with pytest.raises(ValueError, match="gamma must be >= 1/2"):
            HyperNewmarkSolver(m(), loss, 0.1, gamma=0.4)
        for rho in (0.0, -2.0):
            with pytest.raises(ValueError, match="density must be > 0"):
                HyperNewmarkSolver(m(), loss, 0.1, density=rho)
        with pytest.raises(ValueError, match="mass"):
            HyperNewmarkSolver(m(), loss, 0.1, mass="diagonal")
        with pytest.raises(ValueError, match="precond"):
            HyperNewmarkSolver(m(), loss, 0.1, precond="amg_tangent")
        with pytest.raises(ValueError, match="iters_per_graph"):
            HyperNewmarkSolver(m(), loss, 0.1, iters_per_graph=0)
        for eta in (0.0, 1.0):
            with pytest.raises(ValueError, match="eta_max"):
                HyperNewmarkSolver(m(), loss, 0.1, eta_max=eta)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                HyperNewmarkSolver(m(), loss, 0.1)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                hyper_transient_(m(), loss, 2, 0.1, beta=0.0, mass="lumped", precond="none")


def test_step_info_keeps_its_fields_and_gains_three():
    from hidenn_fem_amd.dynamics import HyperStepInfo, StepInfo
    i = HyperStepInfo(t=0.1, iterations=3, residual_norm=1e-9, rhs_norm=1.0, converged=True, reason="rtol")
    assert isinstance(i, StepInfo) and i.newton_iterations == 0 and math.isnan(i.min_J) and i.history == []
