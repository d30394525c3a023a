"""r-adaptive solve (TRI3 and QUAD4): alternate the frozen-mesh displacement solve with inversion-safe coordinate steps.

HiDeNN-FEM treats the nodal coordinates as trainable: the FE energy is lowered by moving the interior nodes.  With the reduced
energy ``Pi*(x) = min_u E(u, x)`` (evaluated by ``solve.FrozenMeshSolver`` / ``solve.Quad4FrozenMeshSolver``), the envelope
theorem gives
``grad Pi*(x) = dE/dx`` at ``u = u*(x)`` -- the coordinate gradient the graded energy kernel already returns.  A step on ``x``
at fixed ``u_k`` that passes an Armijo test gives ``Pi*(x_k+1) <= E(u_k, x_k+1) < E(u_k, x_k) = Pi*(x_k)``: re-solving ``u`` (CG
from ``u_k``, whose energy only decreases) can only lower it further, so every outer iteration lowers the reduced energy.
What keeps each step valid is device code (``csrc/mesh_guard.hip``): the step bound (the largest step before some element
keeps less than ``eta`` of its signed area -- ``detJ(x + a d)`` is an exact quadratic in ``a``), the element measure (signed
mean-ratio quality ``q``, the ``detJ`` ratio to the initial mesh, the inverted count) and the opt-in quality barrier
``Q(x) = (w / Ne) sum (1/q - 1)``: the ``mesh_quality_loss`` the reference's example 4 sketches (examples/example4.py:83-110)
and never defines.

QUAD4 models (the same file): the same three pieces per CORNER of a bilinear cell.  With the corner cross product
``c_k = (X_k+1 - X_k) x (X_k-1 - X_k)`` (``= 4 detJ`` at corner ``k``; ``detJ`` is affine over the reference square, so its
extremes are at the corners) a cell is valid everywhere iff all four ``s c_k > 0``, the step bound is the first step at which
some ``c_k`` keeps only ``eta`` of its value (every Gauss-point ``detJ`` then keeps at least ``eta``), ``q = min_k q_k`` with
``q_k = 2 s c_k / (|X_k+1 - X_k|^2 + |X_k-1 - X_k|^2)`` (1 at a right-angled corner with equal sides), ``det_ratio = min_k
c_k / c_k_initial`` and ``Q(x) = (w / (4 Ne)) sum_e sum_k (1/q_ek - 1)``.

Each function and class takes one element kind: ``RAdaptiveSolver``, ``mesh_quality``, ``max_feasible_step``, ``quality_barrier``
TRI3 models, ``Quad4RAdaptiveSolver``, ``quad4_mesh_quality``, ``quad4_max_feasible_step``, ``quad4_quality_barrier`` QUAD4
models; ``r_adapt_`` takes either.  The outer loop, the line search and the stopping rules are one piece of code
(``_RAdaptBase``).  Coordinate rows fp64 or fp32 (fp64 inside the kernels), any storage row order (``reorder``).

Finite strain (``NeoHookeanLoss2D`` / ``Quad4NeoHookeanLoss2D``): ``HyperRAdaptiveSolver`` and
``Quad4HyperRAdaptiveSolver`` run the same loop with ``newton.NewtonKrylovSolver`` / ``Quad4NewtonKrylovSolver`` as the
displacement solve.  There the quantity that must not collapse is ``det F = detJ(X + u) / detJ(X)``, and a coordinate step at
fixed nodal ``u`` moves numerator and denominator: a trial that keeps the reference area can still drive ``det F`` to zero
and the energy to ``+inf``.  ``csrc/mesh_guard.hip`` holds the guard for both element kinds as well: the step bound that
also stops at the first step with ``det F(a) = eta det F(0)`` (an exact quadratic as well; ``hyper_max_feasible_step``,
``quad4_hyper_max_feasible_step``) and the deformation measure ``J`` (``deformation_measure``,
``quad4_deformation_measure``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from . import _lib
from ._lib import check, dev_index, ptr, stream_ptr
from .loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D

F64 = torch.float64


def _check_eta(eta):
    if not (0.0 < float(eta) < 1.0):
        raise ValueError(f"eta must be in (0, 1), got {eta!r}")


class _Mesh:
    """What the mesh kernels read of a model: the int32 connectivity, the x row map, the fixed and the reference rows (all on
    the model's device, in its coordinate dtype).  TRI3 (``csrc/mesh_guard.hip``); ``_QuadMesh`` is the QUAD4 one."""

    abi, npe, kind = "hfem_tri3", 3, "TRI3"                    # prefix of the three entry points, nodes per element
    other = "QUAD4 models: quad4_mesh_quality, quad4_max_feasible_step, quad4_quality_barrier, Quad4RAdaptiveSolver"
    measure_f32_trials = False                                 # _RAdaptBase._line_search: measure fp32 trials as stored

    @classmethod
    def require(cls, model, what):
        if getattr(model, "nodes_per_element", 3) != cls.npe:
            raise NotImplementedError(f"{what}: {cls.kind} models only ({cls.other}; r_adapt_ takes either kind)")

    def __init__(self, model):
        self.require(model, "hidenn_fem_amd.radapt")
        xf = _lib.require_gpu_tensor(model.node_coords_free, "node_coords_free", dtype=None)
        if xf.dtype not in (F64, torch.float32):
            raise RuntimeError(f"hidenn_fem_amd.radapt: coordinate rows must be fp64 or fp32, got {xf.dtype}")
        self.model, self.dtype, self.device = model, xf.dtype, xf.device
        self.f32 = xf.dtype == torch.float32
        self.ne = int(model.Nelems)
        self.conn = model._conn32.to(self.device).contiguous()
        self.x_src = torch.from_numpy(model._x_src).to(self.device)
        self.x_ref = model.initial_node_coords.to(device=self.device, dtype=self.dtype).contiguous()
        self.n_x = int(xf.shape[0])

    def fixed(self):
        t = self.model.node_coords_fixed.to(device=self.device, dtype=self.dtype).contiguous()
        return t if t.numel() else None

    def _x_rows(self):
        """The x row map and the tensors behind it: the model's CURRENT free rows and its fixed rows (None if there are none)."""
        return self.x_src, self.model.node_coords_free.detach(), self.fixed()

    def _call(self, name, *args, rows=None):
        """Call the entry point ``name`` of this element kind (its ``_f32`` twin for fp32 rows) and check its return code.  Every
        entry point starts with the device, the connectivity, the element count and the row maps with their rows -- ``rows``
        (default ``_x_rows()``), referenced here until the call returns -- and ends with the stream; ``args`` go in between."""
        rows = self._x_rows() if rows is None else rows
        name = f"{self.abi}_{name}"
        fn = getattr(_lib.lib(), name + "_f32" if self.f32 else name)
        check(fn(dev_index(self.device), ptr(self.conn), self.ne, *(ptr(t) for t in rows), *args, stream_ptr(self.device)), name)

    def measure(self, x_ref=None, per_element=True):
        """(q [Ne] or None, ratio [Ne] or None, summary [3] fp64 device) against ``x_ref`` (default: initial coordinates)."""
        dev = self.device
        q = torch.empty(self.ne, dtype=F64, device=dev) if per_element else None
        r = torch.empty(self.ne, dtype=F64, device=dev) if per_element else None
        summary = torch.empty(3, dtype=F64, device=dev)
        xr = self.x_ref if x_ref is None else x_ref.to(dtype=self.dtype).contiguous()
        self._call("mesh_measure", ptr(xr), ptr(q), ptr(r), ptr(summary))
        return q, r, summary

    def step_bound(self, d, eta, out=None):
        """0-d fp64 device tensor: the largest step along ``d`` (fp64 [n_x, 2], storage order) that keeps every element's
        ``detJ`` at or above ``eta`` times its current value."""
        out = torch.empty((), dtype=F64, device=self.device) if out is None else out
        self._call("step_bound", ptr(d), float(eta), ptr(out))
        return out

    def barrier(self, weight, grad=True):
        """(Q 0-d fp64, dQ/dx_free fp64 [n_x, 2] or None) at the current coordinates."""
        dev = self.device
        val = torch.zeros((), dtype=F64, device=dev)
        g = torch.zeros((self.n_x, 2), dtype=F64, device=dev) if grad else None
        self._call("quality_barrier", ptr(self.x_ref), float(weight), ptr(val), ptr(g))
        return val, g

    # ---- the public functions of an element kind
    def quality(self):
        q, r, s = self.measure()
        s = s.tolist()
        return MeshQuality(q=q, det_ratio=r, min_q=s[0], min_det_ratio=s[1], n_inverted=int(s[2]))

    def feasible_step(self, d, eta, as_tensor):
        if tuple(d.shape) != (self.n_x, 2):
            raise ValueError(f"d must have the shape of node_coords_free {(self.n_x, 2)}, got {tuple(d.shape)}")
        d64 = d.detach().to(device=self.device, dtype=F64).contiguous()
        a = self.step_bound(d64, eta)
        return a if as_tensor else a.item()


class _QuadMesh(_Mesh):
    """``_Mesh`` of a QUAD4 model: connectivity ``[Ne, 4]``, the corner-wise kernels of ``csrc/mesh_guard.hip``."""

    abi, npe, kind = "hfem_quad4", 4, "QUAD4"
    other = "TRI3 models: mesh_quality, max_feasible_step, quality_barrier, RAdaptiveSolver"
    measure_f32_trials = True


class _HyperRows:
    """What the finite-strain mesh kernels read besides the coordinates (``csrc/mesh_guard.hip``): the u row map and the
    model's CURRENT ``u_free`` and ``u_fixed_rows()``.  Mixed into a mesh class, it replaces the step bound by the det F-safe
    one and adds the deformation measure; fp32 trials are measured for both element kinds."""

    measure_f32_trials = True

    def __init__(self, model):
        super().__init__(model)
        if model.u_free.dtype != self.dtype or model.u_free.device != self.device:
            raise RuntimeError(f"hidenn_fem_amd.radapt: u_free must have the dtype and device of node_coords_free "
                               f"({self.dtype}, {self.device}), got {model.u_free.dtype}, {model.u_free.device}")
        self.u_src = torch.from_numpy(model._u_src).to(self.device)

    def _xu_rows(self):
        """``_x_rows()``, then the u row map and the tensors behind it: the model's CURRENT ``u_free`` and fixed rows."""
        uf = self.model.u_free.detach().contiguous()
        ufix = self.model.u_fixed_rows().detach().to(device=self.device, dtype=self.dtype).contiguous()
        return self._x_rows() + (self.u_src, uf if uf.numel() else None, ufix if ufix.numel() else None)

    def step_bound(self, d, eta, out=None):
        """0-d fp64 device tensor: the largest step along ``d`` (fp64 [n_x, 2], storage order) at fixed ``u`` that keeps every
        element's (QUAD4: corner's) ``detJ`` and ``det F`` at or above ``eta`` times their current values."""
        out = torch.empty((), dtype=F64, device=self.device) if out is None else out
        self._call("hyper_step_bound", ptr(d), float(eta), ptr(out), rows=self._xu_rows())
        return out

    def deformation(self, per_element=True):
        """(J [Ne] or None, summary [2] fp64 device = {min J, number of elements with J <= 0 or NaN}) at the current rows."""
        j = torch.empty(self.ne, dtype=F64, device=self.device) if per_element else None
        summary = torch.empty(2, dtype=F64, device=self.device)
        self._call("deformation_measure", ptr(j), ptr(summary), rows=self._xu_rows())
        return j, summary

    def deformation_measure(self):
        j, s = self.deformation()
        s = s.tolist()
        return DeformationMeasure(J=j, min_J=s[0], n_inverted=int(s[1]))


class _HyperMesh(_HyperRows, _Mesh):
    other = "QUAD4 models: quad4_hyper_max_feasible_step, quad4_deformation_measure, Quad4HyperRAdaptiveSolver"


class _QuadHyperMesh(_HyperRows, _QuadMesh):
    other = "TRI3 models: hyper_max_feasible_step, deformation_measure, HyperRAdaptiveSolver"


@dataclass
class MeshQuality:
    """Element measure against the model's ``initial_node_coords``.  ``q`` [Ne]: signed mean-ratio quality (1 = equilateral,
    <= 0 = inverted); ``det_ratio`` [Ne]: ``detJ / detJ_initial``; both fp64 on the device, elements in the caller's order.
    From ``quad4_mesh_quality``: the smallest corner value of each (``q`` = 1 for a square, module docstring)."""
    q: torch.Tensor
    det_ratio: torch.Tensor
    min_q: float
    min_det_ratio: float
    n_inverted: int


def mesh_quality(model) -> MeshQuality:
    """Per-element quality and ``detJ`` ratio of the current coordinates, with the minimum of each and the number of inverted
    elements (one measure launch; the summary is reduced on the device, deterministically)."""
    _Mesh.require(model, "mesh_quality")
    return _Mesh(model).quality()


def max_feasible_step(model, d: torch.Tensor, eta: float = 0.25, as_tensor: bool = False):
    """The largest ``alpha`` such that moving the free coordinate rows by ``alpha * d`` keeps every element's signed ``detJ``
    at or above ``eta`` times its current value (``+inf`` if no step along ``d`` gets there).  ``d``: ``[n_x, 2]`` in the
    storage order of ``node_coords_free`` (any float dtype; used in fp64).  For any caller's optimiser: a trial step below it
    cannot invert an element.  ``as_tensor=True`` returns the 0-d fp64 device tensor without a host sync."""
    _Mesh.require(model, "max_feasible_step")
    _check_eta(eta)
    return _Mesh(model).feasible_step(d, eta, as_tensor)


def quality_barrier(model, weight: float = 1.0):
    """``Q = (weight / Ne) sum_e (1/q_e - 1)`` at the current coordinates and its gradient with respect to the free coordinate
    rows (fp64 ``[n_x, 2]``, storage order).  Accumulated with fp64 atomics: not bit-reproducible run to run."""
    _Mesh.require(model, "quality_barrier")
    return _Mesh(model).barrier(weight)


def quad4_mesh_quality(model) -> MeshQuality:
    """``mesh_quality`` for a QUAD4 model: per element the smallest corner quality ``q = min_k q_k`` and the smallest corner
    ratio ``min_k c_k / c_k_initial``, the minimum of each over the mesh and the number of inverted elements (a cell counts
    when any corner has ``s c_k <= 0``: ``detJ`` is then <= 0 somewhere in it).  Deterministic."""
    _QuadMesh.require(model, "quad4_mesh_quality")
    return _QuadMesh(model).quality()


def quad4_max_feasible_step(model, d: torch.Tensor, eta: float = 0.25, as_tensor: bool = False):
    """``max_feasible_step`` for a QUAD4 model: the largest ``alpha`` such that moving the free coordinate rows by
    ``alpha * d`` keeps every corner cross product -- and with them ``detJ`` at every point of every cell -- at or above ``eta``
    times its current value (``+inf`` if no step along ``d`` gets there).  Same arguments and return types."""
    _QuadMesh.require(model, "quad4_max_feasible_step")
    _check_eta(eta)
    return _QuadMesh(model).feasible_step(d, eta, as_tensor)


def quad4_quality_barrier(model, weight: float = 1.0):
    """``Q = (weight / (4 Ne)) sum_e sum_k (1/q_ek - 1)`` over the corners of a QUAD4 model at the current coordinates and its
    gradient with respect to the free coordinate rows (fp64 ``[n_x, 2]``, storage order).  Accumulated with fp64 atomics: not
    bit-reproducible run to run."""
    _QuadMesh.require(model, "quad4_quality_barrier")
    return _QuadMesh(model).barrier(weight)


@dataclass
class DeformationMeasure:
    """Deformation measure of the model's current coordinates and displacements.  ``J`` [Ne] fp64 on the device, elements in
    the caller's order: ``det F = detJ(X + u) / detJ(X)`` of a TRI3 element, the smallest corner ratio ``c_k^def / c_k`` of a
    QUAD4 cell (``det F`` at any point of the cell is a positively weighted mean of the four).  ``min_J``: its minimum;
    ``n_inverted``: the number of elements with ``J <= 0`` or NaN."""
    J: torch.Tensor
    min_J: float
    n_inverted: int


def hyper_max_feasible_step(model, d: torch.Tensor, eta: float = 0.25, as_tensor: bool = False):
    """``max_feasible_step`` at finite strain: the largest ``alpha`` such that moving the free coordinate rows by ``alpha * d``
    AT FIXED NODAL ``u`` (the model's current ``u_free`` and ``u_fixed_rows()``) keeps every element's ``detJ`` and its
    ``det F = detJ(X + u) / detJ(X)`` at or above ``eta`` times their current values (``+inf`` if no step along ``d`` gets
    there, 0 if an element is invalid already).  No Neo-Hookean energy is ``+inf`` below it.  Same arguments and return types."""
    _HyperMesh.require(model, "hyper_max_feasible_step")
    _check_eta(eta)
    return _HyperMesh(model).feasible_step(d, eta, as_tensor)


def quad4_hyper_max_feasible_step(model, d: torch.Tensor, eta: float = 0.25, as_tensor: bool = False):
    """``hyper_max_feasible_step`` for a QUAD4 model, per corner: below it every corner cross product of the reference cell and
    every corner ratio ``c_k^def / c_k`` keep ``eta`` of their values, so ``det F`` at every point of a cell -- every Gauss
    point -- stays at or above ``eta`` times the cell's smallest corner ratio before the step."""
    _QuadHyperMesh.require(model, "quad4_hyper_max_feasible_step")
    _check_eta(eta)
    return _QuadHyperMesh(model).feasible_step(d, eta, as_tensor)


def deformation_measure(model) -> DeformationMeasure:
    """Per-element ``det F`` of a TRI3 model's current state, its minimum and the number of elements with ``det F <= 0`` (one
    measure launch; the summary is reduced on the device, deterministically)."""
    _HyperMesh.require(model, "deformation_measure")
    return _HyperMesh(model).deformation_measure()


def quad4_deformation_measure(model) -> DeformationMeasure:
    """``deformation_measure`` for a QUAD4 model: per cell the smallest corner ratio.  (``Quad4NeoHookeanLoss2D.info`` reports
    the minimum over the Gauss points instead, which is never below it.)"""
    _QuadHyperMesh.require(model, "quad4_deformation_measure")
    return _QuadHyperMesh(model).deformation_measure()


@dataclass
class RAdaptInfo:
    """Outcome of ``RAdaptiveSolver.run()`` / ``Quad4RAdaptiveSolver.run()``, one entry per outer iteration (entry 0: the
    frozen-mesh solve at the start).
    ``energy``: ``Pi*`` (the energy at the solved ``u``); ``objective``: ``Pi* + Q`` (what the line search lowers; equal to
    ``energy`` without the barrier); ``grad_inf``: ``|g_x|_inf`` of the objective; ``alpha`` / ``alpha_max``: the accepted step
    and the step bound (0 / nan at entry 0); ``cg_iterations``; ``min_q`` against the initial mesh; ``step_ratio``: the smallest
    ``detJ(x_k) / detJ(x_k-1)`` over the elements (QUAD4: over their corners; >= ``eta`` by construction); ``trials``:
    line-search evaluations.
    ``reason``: ``"gtol"``, ``"ftol"``, ``"max_outer"``, ``"line_search"`` (no trial passed the Armijo test, not even along the
    steepest descent: the coordinates are left at the last accepted point) or ``"stalled"`` (the accepted step rounded away)."""
    energy: List[float] = field(default_factory=list)
    objective: List[float] = field(default_factory=list)
    grad_inf: List[float] = field(default_factory=list)
    alpha: List[float] = field(default_factory=list)
    alpha_max: List[float] = field(default_factory=list)
    cg_iterations: List[int] = field(default_factory=list)
    min_q: List[float] = field(default_factory=list)
    step_ratio: List[float] = field(default_factory=list)
    trials: List[int] = field(default_factory=list)
    reason: str = ""

    @property
    def iterations(self) -> int:
        return len(self.energy) - 1


class _RAdaptBase:
    """The alternating loop both element kinds share: argument checks, the pieces of an outer iteration, the L-BFGS direction,
    the line search and ``run``.  A subclass names its mesh class (``_mesh_cls``: which models it takes and which mesh kernels
    run) and its displacement solver (``_solver_cls()``), and may refuse more in ``_check``.  The finite-strain classes
    (``_HyperRAdaptBase``) also replace ``solve_and_grad`` and the small hooks ``_step_start`` / ``_trial_share`` /
    ``_step_extra`` / ``_record_extra`` / ``_solve_failed``, which do nothing more here than the loop always did."""

    _mesh_cls = None
    _info_cls = RAdaptInfo

    @staticmethod
    def _solver_cls():
        raise NotImplementedError

    @classmethod
    def _check(cls, model, loss_fn):
        cls._mesh_cls.require(model, cls.__name__)
        if getattr(loss_fn, "elastoplastic", False):
            raise NotImplementedError(f"{cls.__name__}: small-strain linear elasticity only; a J2PlasticityLoss2D has a history "
                                      "on the mesh it was loaded on -- no r-adaptation under plasticity; its load path is "
                                      "hidenn_fem_amd.plasticity.ElastoplasticSolver")
        if isinstance(loss_fn, NeoHookeanLoss2D):
            raise NotImplementedError(f"{cls.__name__}: small-strain linear elasticity only (its frozen-mesh solve would "
                                      "linearise a NeoHookeanLoss2D silently); finite strain: HyperRAdaptiveSolver (TRI3) / "
                                      "Quad4HyperRAdaptiveSolver (QUAD4), or r_adapt_, which picks the class")
        if getattr(loss_fn, "deterministic", False):
            raise NotImplementedError(f"{cls.__name__}: EnergyLoss2D(deterministic=True) has no solver counterpart "
                                      "(the CG matrix-vector product accumulates with LDS atomics)")

    def __init__(self, model, loss_fn, b_force: Optional[Callable] = None, t_force: Optional[Callable] = None, *,
                 history: int = 10, eta: float = 0.25, quality_weight: float = 0.0, cg_rtol: float = 1e-10,
                 gtol: float = 1e-9, ftol: float = 1e-12, max_outer: int = 50, max_ls: int = 20, c1: float = 1e-4,
                 max_restarts: int = 5, cg_precond: str = "block_jacobi"):
        self._check(model, loss_fn)
        if int(max_restarts) < 0:
            raise ValueError("max_restarts must be >= 0")
        self._setup(model, loss_fn, b_force, t_force, history, eta, quality_weight, gtol, ftol, max_outer, max_ls, c1)
        self.max_restarts = int(max_restarts)
        self.solver = self._solver_cls()(model, loss_fn, b_force=b_force, t_force=t_force, rtol=cg_rtol,
                                         precond=cg_precond)

    def _setup(self, model, loss_fn, b_force, t_force, history, eta, quality_weight, gtol, ftol, max_outer, max_ls, c1):
        """Everything of ``__init__`` after ``_check`` but the displacement solver."""
        _check_eta(eta)
        if int(history) < 0 or int(max_outer) < 0 or int(max_ls) < 1:
            raise ValueError("history and max_outer must be >= 0, max_ls >= 1")
        if not (0.0 < c1 < 1.0):
            raise ValueError("c1 must be in (0, 1)")
        if not (quality_weight >= 0.0 and math.isfinite(quality_weight)):
            raise ValueError("quality_weight must be finite and >= 0")
        if gtol < 0 or ftol < 0:
            raise ValueError("gtol and ftol must be >= 0")
        self.mesh = self._mesh_cls(model)
        self.model, self.loss_fn, self.b_force, self.t_force = model, loss_fn, b_force, t_force
        self.history, self.eta, self.quality_weight = int(history), float(eta), float(quality_weight)
        self.gtol, self.ftol, self.max_outer, self.max_ls, self.c1 = float(gtol), float(ftol), int(max_outer), int(max_ls), float(c1)
        self.last_solve = None                                 # SolveInfo of the latest displacement solve
        x0 = model.initial_node_coords.detach().double()
        self.length = float((x0.max(dim=0).values - x0.min(dim=0).values).norm()) if x0.numel() else 1.0

    # ---- pieces of an outer iteration (also timed one by one by scripts/radapt_timing.py)
    def objective_and_grad(self):
        """(``E``, ``E + Q``, flat fp64 ``d(E + Q)/dx_free``, ``||dE/du_free||``) at the current ``u`` and coordinates (one
        launch yields both gradients); ``.grad`` untouched."""
        m = self.model
        with torch.enable_grad():
            e = self.loss_fn(m, self.b_force, self.t_force)
            gx, gu = torch.autograd.grad(e, [m.node_coords_free, m.u_free])
        self._gu_norm = float(gu.detach().double().norm().item())
        g = gx.detach().to(F64).reshape(-1)
        e = float(e.detach().double().item())
        f = e
        if self.quality_weight > 0.0:
            q, gq = self.mesh.barrier(self.quality_weight)
            g = g + gq.reshape(-1)
            f = e + float(q.item())
        return e, f, g

    def solve_and_grad(self):
        """Displacement solve at the current coordinates, then ``objective_and_grad()``.  fp64 models: while the true residual
        ``||dE/du||`` exceeds twice the CG tolerance, CG restarts from the current ``u`` (at most ``max_restarts`` times).  The
        solver's own test reads the recurrence residual, which drifts from the true one by about eps x cond(K) -- and cond(K)
        grows as r-adaptation thins elements (1/min q).  Returns (E, E + Q, g, CG iterations)."""
        sol = self.last_solve = self.solver.solve()
        iters = sol.iterations
        e, f, g = self.objective_and_grad()
        if self.model.node_coords_free.dtype == F64:                # fp32 rows: rounding u on write-back sets the floor
            for _ in range(self.max_restarts):
                before = self._gu_norm
                if not before > 2.0 * self.solver.rtol * sol.rhs_norm:
                    break
                sol = self.last_solve = self.solver.solve()
                iters += sol.iterations
                e, f, g = self.objective_and_grad()
                if not self._gu_norm < 0.5 * before:                   # at the rounding floor: restarts no longer help
                    break
        return e, f, g, iters

    def objective(self) -> float:
        """``E + Q`` at the current ``u`` and coordinates, loss only."""
        with torch.no_grad():
            f = float(self.loss_fn(self.model, self.b_force, self.t_force).double().item())
            if self.quality_weight > 0.0:
                f += float(self.mesh.barrier(self.quality_weight, grad=False)[0].item())
        return f

    def _direction(self, g, pairs):
        """L-BFGS two-loop recursion over the flat x rows: ``d = -H g``."""
        q = -g
        if not pairs:
            return q
        alphas = []
        for s, y, rho in reversed(pairs):
            a = rho * torch.dot(s, q)
            q = q - a * y
            alphas.append(a)
        s, y, _ = pairs[-1]
        q = q * (torch.dot(s, y) / torch.dot(y, y))
        for (s, y, rho), a in zip(pairs, reversed(alphas)):
            b = rho * torch.dot(y, q)
            q = q + (a - b) * s
        return q

    def _step_start(self):
        """What ``_trial_share`` and ``_step_extra`` need of ``x_k`` besides its coordinates (taken before the rows move)."""
        return None

    def _trial_share(self, coords0, start) -> float:
        """The smallest share the rows as stored keep of what the step bound protects, against ``x_k`` (``coords0``)."""
        return float(self.mesh.measure(x_ref=coords0, per_element=False)[2][1].item())

    def _step_extra(self, start):
        """What a subclass records of an accepted step besides ``step_ratio`` (before ``u`` is solved again)."""
        return None

    def _record_extra(self, info, extra):
        pass

    def _solve_failed(self) -> bool:
        """The latest displacement solve left a state the outer loop must not continue from."""
        return False

    def _line_search(self, x0, d, f0, gd, alpha_init, coords0=None, start=None):
        """Backtracking Armijo along ``d`` from the rows ``x0`` (fp64 flat).  Returns (accepted alpha or None, alpha_max, f, trials);
        on failure ``node_coords_free`` holds ``x0`` again.  fp32 rows of a mesh class with ``measure_f32_trials`` (QUAD4 and
        the finite-strain classes; ``coords0`` is ``x0`` by node id, ``start`` is ``_step_start()`` there): the step bound
        holds for ``x0 + alpha d``, the rows hold that rounded, and on an element that earlier steps shrank to the spacing of
        the float grid the rounding moves ``detJ`` by more than the 0.9 margin leaves.  So each trial is measured against
        ``coords0`` first, and one that keeps less than ``eta`` is halved like one that fails the Armijo test (it counts as
        a trial; the energy is not evaluated)."""
        xf = self.model.node_coords_free
        d2 = d.reshape(xf.shape).contiguous()
        amax = float(self.mesh.step_bound(d2, self.eta).item())
        alpha = min(alpha_init, 0.9 * amax)
        if not math.isfinite(alpha):                          # no element shrinks along d and no curvature yet
            alpha = 1.0
        measured = self.mesh.f32 and self.mesh.measure_f32_trials and coords0 is not None
        for t in range(self.max_ls):
            with torch.no_grad():
                xf.copy_((x0 + alpha * d).reshape(xf.shape))   # rounds once for fp32 rows
            kept = not measured or self._trial_share(coords0, start) >= self.eta
            f = self.objective() if kept else math.inf
            if math.isfinite(f) and f <= f0 + self.c1 * alpha * gd:
                return alpha, amax, f, t + 1
            alpha *= 0.5
        with torch.no_grad():
            xf.copy_(x0.reshape(xf.shape))
        return None, amax, f0, self.max_ls

    def run(self) -> RAdaptInfo:
        m, info = self.model, self._info_cls()
        xf = m.node_coords_free
        e, f, g, cg_iters = self.solve_and_grad()
        gscale = max(abs(f), 1e-300) / self.length

        def record(e, f, g, alpha, amax, cg_iters, step_ratio, trials, extra=None):
            _, _, s = self.mesh.measure(per_element=False)
            info.energy.append(e)
            info.objective.append(f)
            info.grad_inf.append(float(g.abs().max().item()) if g.numel() else 0.0)
            info.alpha.append(alpha)
            info.alpha_max.append(amax)
            info.cg_iterations.append(cg_iters)
            info.min_q.append(float(s[0].item()))
            info.step_ratio.append(step_ratio)
            info.trials.append(trials)
            self._record_extra(info, extra)

        record(e, f, g, 0.0, math.nan, cg_iters, math.nan, 0)
        pairs, last = [], None                                 # curvature pairs (s, y, 1 / s^T y); the latest pair for BB
        while True:
            if self._solve_failed():
                info.reason = "newton"
                break
            if info.grad_inf[-1] <= self.gtol * gscale:
                info.reason = "gtol"
                break
            if info.iterations >= self.max_outer:
                info.reason = "max_outer"
                break
            x0 = xf.detach().to(F64).reshape(-1).clone()
            with torch.no_grad():
                coords0 = m.coords.to(self.mesh.dtype).contiguous()     # x_k by node id: the reference of the step ratio
            start = self._step_start()
            step = None
            for use_pairs in ([True, False] if pairs else [False]):   # L-BFGS direction, then once the steepest descent
                d = self._direction(g, pairs if use_pairs else [])
                gd = float(torch.dot(g, d).item())
                if not gd < 0.0:                                    # not a descent direction: steepest descent instead
                    d, gd, use_pairs = -g, -float(torch.dot(g, g).item()), False
                if use_pairs:
                    alpha_init = 1.0
                elif last is not None:
                    sy = float(torch.dot(last[0], last[1]).item())
                    alpha_init = float(torch.dot(last[0], last[0]).item()) / sy if sy > 0.0 else math.inf
                else:
                    alpha_init = math.inf
                alpha, amax, _, trials = self._line_search(x0, d, f, gd, alpha_init, coords0, start)
                if alpha is not None:
                    step = (alpha, amax, trials)
                    break
                pairs = []                                          # the curvature history did not help: drop it
                if not use_pairs:
                    break
            if step is None:
                info.reason = "line_search"
                break
            x1 = xf.detach().to(F64).reshape(-1)
            if torch.equal(x1, x0):
                info.reason = "stalled"
                break
            _, ratio, _ = self.mesh.measure(x_ref=coords0)
            step_ratio = float(ratio.min().item()) if ratio.numel() else math.nan
            extra = self._step_extra(start)
            e1, f1, g1, cg_iters = self.solve_and_grad()
            s, y = x1 - x0, g1 - g
            sy = float(torch.dot(s, y).item())
            if sy > 0.0:
                last = (s, y)
                if self.history > 0:
                    pairs.append((s, y, 1.0 / sy))
                    pairs = pairs[-self.history:]
            record(e1, f1, g1, step[0], step[1], cg_iters, step_ratio, step[2], extra)
            f_old, f, g = f, f1, g1
            if f_old - f1 <= self.ftol * max(abs(f_old), abs(f1), 1.0):
                info.reason = "ftol"
                break
        return info


class RAdaptiveSolver(_RAdaptBase):
    """Alternating r-adaptive minimisation of the TRI3 energy over ``u_free`` and ``node_coords_free`` (module docstring).

    One outer iteration: (1) ``u <- FrozenMeshSolver.solve()``, warm-started (one solver instance; it refreshes itself when the
    coordinates moved; fp64 models restart it from the true residual when that drifted, ``solve_and_grad``); (2) ``g_x = dE/dx_free`` at that ``u`` through ``loss_fn(model, b_force, t_force)`` and
    ``torch.autograd.grad`` on ``node_coords_free`` alone (every force table enters as in training), plus ``dQ/dx`` when
    ``quality_weight > 0``; (3) an L-BFGS direction over the x rows (``history`` pairs, a pair with ``s^T y <= 0`` skipped;
    ``history=0``: steepest descent with a Barzilai-Borwein initial step); (4) ``alpha_max`` from the step-bound kernel, trial
    ``min(alpha_init, 0.9 alpha_max)`` (``alpha_init`` = 1 with curvature pairs, the BB step without, ``0.9 alpha_max`` at the
    very first step), halved until ``E(u_k, x + a d) + Q(x + a d)`` passes the Armijo test with ``c1`` -- one loss-only
    evaluation per trial, ``x + a d`` written into ``node_coords_free`` in place.  A failed search retries once along the
    steepest descent, then restores ``x`` and stops.

    Stopping: ``gtol`` -- ``|g_x|_inf <= gtol * |Pi*_0 + Q_0| / L`` (``L``: diagonal of the initial mesh's bounding box, so the
    test is free of units); ``ftol`` -- the objective fell by no more than ``ftol * max(|f_k|, |f_k+1|, 1)``; ``max_outer``
    coordinate steps.  Only ``node_coords_free`` and ``u_free`` change: ``.grad`` of both, the Dirichlet rows and the fixed
    coordinate rows are untouched.  fp32 models: fp64 inside the kernels, coordinates rounded once per trial on write-back (the
    0.9 margin and ``eta`` absorb the rounding).  QUAD4 models (``Quad4RAdaptiveSolver``, or ``r_adapt_``, which takes either)
    and ``EnergyLoss2D(deterministic=True)`` are refused.
    ``cg_precond`` is the ``precond`` of the inner ``FrozenMeshSolver`` (``"amg"``: the AMG host setup is done once, every
    coordinate step redoes only its numeric setup)."""

    _mesh_cls = _Mesh

    @staticmethod
    def _solver_cls():
        from .solve import FrozenMeshSolver
        return FrozenMeshSolver


class Quad4RAdaptiveSolver(_RAdaptBase):
    """``RAdaptiveSolver`` for QUAD4 models (``QuadShapeNN2D``): the same arguments, the same ``RAdaptInfo``, the same outer
    loop, line search and stopping rules (one piece of code).  The displacement solve is ``Quad4FrozenMeshSolver``; the step
    bound, the measure and the opt-in barrier are the corner-wise kernels of ``csrc/mesh_guard.hip`` (module docstring): a step
    keeps every corner cross product, and so ``detJ`` at every Gauss point, at or above ``eta`` of its value, and
    ``step_ratio`` is the smallest corner ratio.  fp32 models: each rounded trial of the line search is measured against
    ``x_k`` and halved while it keeps less than ``eta`` (``_line_search``), so the bound holds for the rows as stored.  Refuses TRI3 models, ``EnergyLoss2D(deterministic=True)`` and the planless
    cross-check path (``loss_fn.quad4_planless``: the CG kernels run on the tile plan)."""

    _mesh_cls = _QuadMesh

    @staticmethod
    def _solver_cls():
        from .solve import Quad4FrozenMeshSolver
        return Quad4FrozenMeshSolver

    @classmethod
    def _check(cls, model, loss_fn):
        super()._check(model, loss_fn)
        if getattr(loss_fn, "quad4_planless", False):
            raise NotImplementedError("Quad4RAdaptiveSolver: quad4_planless=True has no solver counterpart (the CG kernels run "
                                      "on the tile plan)")


@dataclass
class HyperRAdaptInfo(RAdaptInfo):
    """``RAdaptInfo`` of ``HyperRAdaptiveSolver.run()`` / ``Quad4HyperRAdaptiveSolver.run()``.  ``cg_iterations`` is the CG total
    of the entry's Newton solve; added per entry: ``newton_iterations``; ``min_J``, the smallest ``det F`` of the solved state
    as the Newton solve reports it (QUAD4: over the Gauss points); ``J_step_ratio``, the smallest ``J(x_k) / J(x_k-1)`` over
    the elements at the ``u`` the step was taken at, ``J`` from the deformation measure (>= ``eta`` by construction; nan at
    entry 0).  One more ``reason``: ``"newton"`` -- a Newton solve ended unconverged; the state is kept (it is valid, and its
    energy is not above the line search's)."""
    newton_iterations: List[int] = field(default_factory=list)
    min_J: List[float] = field(default_factory=list)
    J_step_ratio: List[float] = field(default_factory=list)


class _HyperRAdaptBase(_RAdaptBase):
    """``_RAdaptBase``'s loop at finite strain: what differs is the displacement solve (Newton-Krylov, no restart
    loop: Newton tests the true gradient), the step bound (the mesh class's det F-safe one), what an fp32 trial is measured
    for (the reference ratio AND the ``J`` ratio against ``x_k``) and the record (``HyperRAdaptInfo``)."""

    _info_cls = HyperRAdaptInfo
    _loss_cls, _wrong_loss, _sibling = NeoHookeanLoss2D, (), ""

    @classmethod
    def _check(cls, model, loss_fn):
        name, npe = cls.__name__, cls._mesh_cls.npe
        if not isinstance(loss_fn, NeoHookeanLoss2D):
            linear = "Quad4RAdaptiveSolver" if npe == 4 else "RAdaptiveSolver"
            raise NotImplementedError(f"{name}: {cls._loss_cls.__name__} only (an EnergyLoss2D is quadratic in u_free: "
                                      f"{linear} alternates with the frozen-mesh PCG solve; r_adapt_ picks the class)")
        if getattr(model, "nodes_per_element", 3) != npe or not isinstance(loss_fn, cls._loss_cls) \
                or isinstance(loss_fn, cls._wrong_loss):
            raise NotImplementedError(f"{name}: {cls._mesh_cls.kind} models under a {cls._loss_cls.__name__} only "
                                      f"({cls._sibling}; r_adapt_ picks the class)")

    def __init__(self, model, loss_fn, b_force: Optional[Callable] = None, t_force: Optional[Callable] = None, *,
                 history: int = 10, eta: float = 0.25, quality_weight: float = 0.0, precond: str = "block_jacobi",
                 newton_rtol: float = 1e-8, newton_kw: Optional[dict] = None, gtol: float = 1e-9, ftol: float = 1e-12,
                 max_outer: int = 50, max_ls: int = 20, c1: float = 1e-4):
        self._check(model, loss_fn)
        self._setup(model, loss_fn, b_force, t_force, history, eta, quality_weight, gtol, ftol, max_outer, max_ls, c1)
        self.solver = self._solver_cls()(model, loss_fn, b_force=b_force, t_force=t_force, precond=precond, rtol=newton_rtol,
                                         **(newton_kw or {}))

    def solve_and_grad(self):
        """Newton-Krylov from the current ``u`` at the current coordinates (the solver refreshes itself when they moved), then
        ``objective_and_grad()``.  Returns (E, E + Q, g, CG iterations of the Newton solve)."""
        sol = self.last_solve = self.solver.solve()
        if sol.reason == "inverted":
            raise RuntimeError(f"{type(self).__name__}: the starting state is inverted (min_J = {sol.min_J!r}): no coordinate "
                               "step is safe from it -- ramp the load to a valid equilibrium first")
        e, f, g = self.objective_and_grad()
        return e, f, g, sol.cg_iterations

    def _solve_failed(self):
        return not self.last_solve.converged

    def _step_start(self):
        return self.mesh.deformation()[0]                       # J per element at (x_k, u_k)

    def _j_ratio(self, start) -> float:
        j = self.mesh.deformation()[0]
        return float((j / start).min().item()) if j.numel() else math.inf

    def _trial_share(self, coords0, start):
        return min(super()._trial_share(coords0, start), self._j_ratio(start))

    def _step_extra(self, start):
        return self._j_ratio(start)

    def _record_extra(self, info, extra):
        info.newton_iterations.append(self.last_solve.newton_iterations)
        info.min_J.append(self.last_solve.min_J)
        info.J_step_ratio.append(math.nan if extra is None else extra)


class HyperRAdaptiveSolver(_HyperRAdaptBase):
    """Alternating r-adaptive minimisation of the Neo-Hookean potential of a TRI3 model over ``u_free`` and
    ``node_coords_free``: ``RAdaptiveSolver``'s outer loop, L-BFGS direction, line search and stopping rules (one piece of
    code), with four differences.

    (1) The displacement solve is ``NewtonKrylovSolver``, warm-started from ``u_k``; it refreshes itself when the coordinates
    moved.  ``precond`` is its ``precond`` (``"block_jacobi"``, ``"none"``, ``"amg"``, ``"amg_tangent"``), ``newton_rtol`` its
    ``rtol``, ``newton_kw`` further keywords.  There is no restart loop: Newton tests the true gradient.  (2) The step bound is
    the finite-strain one (``hyper_max_feasible_step``): below it every element keeps ``eta`` of its ``detJ`` and of its
    ``det F`` at the fixed ``u_k``, so no trial energy is ``+inf``.  (3) fp32 rows: each rounded trial is measured against
    ``x_k`` with the mesh measure and the deformation measure and halved while either ratio is below ``eta``.  (4) ``run()``
    returns a ``HyperRAdaptInfo``.

    Every accepted Newton step passes an Armijo test on the energy, so the descent argument of the small-strain loop holds
    and the recorded objectives fall monotonically even where the tangent is indefinite; ``Pi*`` is then the energy of the
    LOCAL minimum Newton reaches from ``u_k``, no more.  A start with ``det F <= 0`` somewhere raises ``RuntimeError`` (it names
    ``min_J``); a Newton solve that ends unconverged after an accepted step stops the run with ``reason="newton"`` and keeps
    that state.  Only ``node_coords_free`` and ``u_free`` change.  Refuses an ``EnergyLoss2D`` (``RAdaptiveSolver``) and QUAD4
    models or losses (``Quad4HyperRAdaptiveSolver``)."""

    _mesh_cls = _HyperMesh
    _wrong_loss = Quad4NeoHookeanLoss2D
    _sibling = "QUAD4 models under a Quad4NeoHookeanLoss2D: Quad4HyperRAdaptiveSolver"

    @staticmethod
    def _solver_cls():
        from .newton import NewtonKrylovSolver
        return NewtonKrylovSolver


class Quad4HyperRAdaptiveSolver(_HyperRAdaptBase):
    """``HyperRAdaptiveSolver`` for QUAD4 models under a ``Quad4NeoHookeanLoss2D``: the same arguments, loop and
    ``HyperRAdaptInfo``.  The displacement solve is ``Quad4NewtonKrylovSolver``; the step bound and the deformation measure are
    the corner-wise kernels of ``csrc/mesh_guard.hip``: a step keeps ``eta`` of every corner cross product and of every
    corner ratio ``c_k^def / c_k``, so ``det F`` at every Gauss point stays at or above ``eta`` times the cell's smallest corner
    ratio before the step; ``J_step_ratio`` is taken on the cells' smallest corner ratios.  Refuses an ``EnergyLoss2D``
    (``Quad4RAdaptiveSolver``) and TRI3 models or losses (``HyperRAdaptiveSolver``)."""

    _mesh_cls = _QuadHyperMesh
    _loss_cls = Quad4NeoHookeanLoss2D
    _sibling = "TRI3 models under a NeoHookeanLoss2D: HyperRAdaptiveSolver"

    @staticmethod
    def _solver_cls():
        from .newton import Quad4NewtonKrylovSolver
        return Quad4NewtonKrylovSolver


def r_adapt_(model, loss_fn, **kw) -> RAdaptInfo:
    """One-shot ``RAdaptiveSolver(model, loss_fn, **kw).run()`` -- ``Quad4RAdaptiveSolver`` for a QUAD4 model, and for a
    ``NeoHookeanLoss2D`` the finite-strain classes ``HyperRAdaptiveSolver`` / ``Quad4HyperRAdaptiveSolver``:
    ``model.node_coords_free`` and ``model.u_free`` are r-adapted in place."""
    quad = getattr(model, "nodes_per_element", 3) == 4
    if isinstance(loss_fn, NeoHookeanLoss2D):
        cls = Quad4HyperRAdaptiveSolver if quad else HyperRAdaptiveSolver
    else:
        cls = Quad4RAdaptiveSolver if quad else RAdaptiveSolver
    return cls(model, loss_fn, **kw).run()
