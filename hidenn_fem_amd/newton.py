"""Newton-Krylov equilibrium solve of a Neo-Hookean TRI3 or QUAD4 model at its CURRENT coordinates.

``NeoHookeanLoss2D`` is not quadratic in the displacements, so its minimum over ``u_free`` is a nonlinear system
``g(u) = dPi/du_free = 0``.  ``NewtonKrylovSolver`` solves it by inexact Newton: every iteration solves ``K_T(u) d = -g(u)`` on
the tangent ``K_T = d2Pi/du2`` by matrix-free preconditioned CG on the GPU -- the PCG driver of the frozen-mesh solve
(``csrc/cg.hip``: vector kernels, device-side scalars, halt, graph replay) with the tangent as its third element kind
(``csrc/tri3_hyper_cg.hip``; ``Quad4NewtonKrylovSolver``: the fourth, ``csrc/quad4_hyper_cg.hip``) -- to the relative
tolerance ``eta_k`` of Eisenstat-Walker choice 2, then backtracks on the energy.
Residual and energy come from ONE launch of the Neo-Hookean energy kernel on the solver's buffers, on the plan the tangent
kernels run on; the launch that evaluates an accepted trial point also delivers the next iteration's gradient.

The tangent can be indefinite (a strongly deformed start).  The driver's breakdown halt -- ``p^T K p <= 0``, detected before
the iterate moves -- is then the truncation rule of truncated Newton: the direction reached so far is taken; if CG broke down
at its iteration 0, the preconditioned steepest-descent direction ``-M g``.  A CG ``max_iter`` halt also takes the direction
reached.  Both are documented behaviour, not errors; with a positive definite preconditioner every such direction descends.

``assemble_tangent`` returns K_T itself as a sparse matrix, and ``precond="amg_tangent"`` builds the AMG hierarchy on it
(DESIGN 21), with fallbacks to the small-strain hierarchy where K_T is not positive definite.

Not deterministic: the LDS atomics of the matrix-vector product make iterates differ in the last bits from run to run.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
from .solve import (F64, HFEM_FLAG_NO_EDGES, HFEM_FLAG_NO_GX, ST_HALTED, ST_ITER, ST_REASON, _AmgDevice, _Frozen, _REASONS,
                    amg_host)

_AMG_PRECONDS = ("amg", "amg_tangent")

EPS = 2.2e-16


@dataclass
class NewtonInfo:
    """Outcome of ``NewtonKrylovSolver.solve()``.  ``grad_norm``: ||g||_2 over the free u rows at the returned state;
    ``rhs_norm``: ||g(u_free = 0)||_2 (``SolveInfo.rhs_norm``'s definition: the loads and the ``u_fixed`` term);
    ``cg_iterations``: the total over all Newton iterations; ``min_J``: the smallest det F of the returned state;
    ``reason``: ``"rtol"`` / ``"atol"`` (||g|| <= max(rtol ||g(0)||, atol), whichever was the larger), ``"max_newton"``,
    ``"line_search"`` (no step length passed the sufficient-decrease test) or ``"inverted"`` (the starting state has an element
    with J <= 0: ``u_free`` was not touched).  ``history``: one dict per Newton iteration -- ``energy`` and ``grad_norm`` at
    its start, the forcing term ``eta``, ``cg_iterations`` and ``cg_reason`` (``"rtol"``, ``"max_iter"``, ``"breakdown"``) of its
    inner solve, the accepted ``step`` t (0 when none was) and ``min_J`` of the accepted state; with ``precond="amg_tangent"``
    only, ``amg``: ``"tangent"`` or ``"small_strain"``, the hierarchy that preconditioned the inner solve whose direction
    was taken."""
    newton_iterations: int
    cg_iterations: int
    grad_norm: float
    rhs_norm: float
    energy: float
    min_J: float
    converged: bool
    reason: str
    history: List[dict] = field(default_factory=list)


class _NewtonSolverBase:
    """What ``NewtonKrylovSolver`` (TRI3) and ``Quad4NewtonKrylovSolver`` share: everything but the model/loss check, the plan,
    the body-force table and the energy launch (``_check_model``, ``_make_plan``, ``_body``, ``_energy``) -- the Newton loop,
    refresh, graph replay, the preconditioners, ``apply``, ``info`` and the meaning of every keyword.

    ``b_force`` / ``t_force``: the callables ``loss_fn(model, b_force, t_force)`` would take (default forces when None),
    tabulated as the loss does and frozen at the current coordinates.  ``precond``: ``"block_jacobi"`` (the tangent's 2x2
    diagonal blocks, rebuilt every Newton iteration; a block that is not positive definite is the identity), ``"none"``, or
    ``"amg"`` (the smoothed-aggregation hierarchy of the SMALL-STRAIN operator at the current coordinates, material
    ``(lambda + 2 mu, lambda, lambda + 2 mu, mu)``: set up once per refresh, a fixed SPD preconditioner for the varying
    tangent; needs Dirichlet rows), or ``"amg_tangent"`` (the same hierarchy, on the same handle, of the ASSEMBLED
    tangent K_T(u_k) with the rigid modes at the deformed position; needs Dirichlet rows.  ``amg_rebuild="newton"``: a
    numeric setup at every linearisation; ``"solve"``: at the first inner solve of each ``solve()`` only -- for load ramps
    that start from the last equilibrium.  K_T can be indefinite, so two safeguards fall back to the small-strain numbers
    of ``"amg"`` on the same handle: (a) when the Cholesky factorisation of the symmetrised coarsest matrix fails, the
    small-strain setup replaces the tangent setup for this linearisation; (b) when an inner solve under the tangent
    hierarchy ends with ``g.d >= 0`` or a non-finite value, the small-strain setup is made and that inner solve is repeated
    once, its iterations added.  ``solver.amg`` reports ``tangent_setups``, ``fallbacks_coarse`` and
    ``fallbacks_descent``).  Newton stops at ``||g|| <= max(rtol ||g(u_free = 0)||, atol)``, tested first in every
    iteration, or after ``max_newton`` iterations.  Inner solve: ``K_T d = -g`` from ``d = 0`` to ``||r|| <= eta_k ||g||``,
    ``eta_0 = eta_max``, ``eta_k = clamp(0.9 (||g_k|| / ||g_k-1||)^2, 1e-12, eta_max)``, at most ``cg_max_iter`` iterations
    (None = ``max(1000, 4 x free nodes)``), ``iters_per_graph`` per graph replay.  Line search: ``t = 1, 1/2, ...`` (at most
    ``max_backtracks`` halvings), accepted when the trial energy is finite and
    ``Pi(u + t d) <= Pi(u) + armijo t g.d + 4 eps |Pi(u)|`` -- the last term keeps the test meaningful once the predicted
    decrease falls below the rounding of Pi; ``+inf`` from an inverted trial state is an ordinary rejection.

    ``solve()`` starts from the current ``model.u_free``, writes the result into it in place and returns a ``NewtonInfo``.
    Coordinates, ``.grad`` of both parameters and the Dirichlet rows are never written.  Solver-owned fp64 buffers: an fp32
    model's rows are widened once per refresh and ``u_free`` is rounded once on write-back.  ``refresh()`` runs by itself
    when the coordinate rows or ``u_fixed`` changed (``_version``, pointer, shape, dtype).  ``apply``, ``linear_solve`` and
    ``diag`` are test and measurement helpers."""

    def __init__(self, model, loss_fn, b_force: Optional[Callable] = None, t_force: Optional[Callable] = None,
                 precond: str = "block_jacobi", rtol: float = 1e-8, atol: float = 0.0, max_newton: int = 50,
                 cg_max_iter: Optional[int] = None, iters_per_graph: int = 16, eta_max: float = 0.1, armijo: float = 1e-4,
                 max_backtracks: int = 30, amg_rebuild: str = "newton"):
        self._check_model(model, loss_fn)
        if precond not in ("block_jacobi", "none") + _AMG_PRECONDS:
            raise ValueError("precond must be 'block_jacobi', 'none', 'amg' or 'amg_tangent'")
        if precond in _AMG_PRECONDS and int(model._idx_udir.shape[0]) == 0:
            raise ValueError(f"precond='{precond}' needs Dirichlet rows: without them the small-strain operator is singular")
        if amg_rebuild not in ("newton", "solve"):
            raise ValueError("amg_rebuild must be 'newton' or 'solve'")
        if int(iters_per_graph) < 1:
            raise ValueError("iters_per_graph must be >= 1")
        if rtol < 0 or atol < 0:
            raise ValueError("rtol and atol must be >= 0")
        if not 0.0 < eta_max < 1.0:
            raise ValueError("eta_max must be in (0, 1)")
        for name, t in (("node_coords_free", model.node_coords_free), ("u_free", model.u_free)):
            _lib.require_gpu_tensor(t, name, dtype=None)
        self.model, self.loss_fn = model, loss_fn
        self.b_force, self.t_force = b_force, t_force
        self.precond, self.rtol, self.atol = precond, float(rtol), float(atol)
        self.max_newton, self.iters_per_graph = int(max_newton), int(iters_per_graph)
        self.eta_max, self.armijo, self.max_backtracks = float(eta_max), float(armijo), int(max_backtracks)
        self.plan = self._make_plan(model, loss_fn)      # the energy launch's plan: shared row maps
        dev = model.u_free.device
        self.device = dev
        self.n_u = int(model.u_free.shape[0])
        self.cg_max_iter = max(1000, 4 * self.n_u) if cg_max_iter is None else int(cg_max_iter)
        h = C.c_void_p()
        check(_lib.lib().hfem_cg_create_hyper(self.plan.handle, self.n_u, C.byref(h)), "hfem_cg_create_hyper")
        self._h = h
        z = dict(dtype=F64, device=dev)
        rows = (self.n_u, 2)
        self._xf = torch.empty(model.node_coords_free.shape, **z)
        self._xfix = torch.empty(model.node_coords_fixed.shape, **z)
        self._ufix = torch.empty((int(model._idx_udir.shape[0]), 2), **z)
        self._u = torch.zeros(rows, **z)               # the current state = the linearisation point the driver is bound to
        self._trial = torch.zeros(rows, **z)
        self._delta = torch.zeros(rows, **z)
        self._zero = torch.zeros(rows, **z)
        self._g = torch.zeros(rows, **z)
        self._gt = torch.zeros(rows, **z)
        self._gz = torch.zeros(rows, **z)
        self._out = torch.zeros(3, **z)                # {Pi, min J, inverted count} of the last energy launch
        self._info = torch.zeros(2, **z)               # {min J, inverted count} of the last linearisation
        self._work = torch.empty(3 * max(self.plan.n_tiles, 1), **z)
        self.diag = torch.zeros((self.n_u, 3), **z)    # the 2x2 diagonal blocks {K_xx, K_xy, K_yy} of the last linearisation
        self._lame = (C.c_double * 2)(*loss_fn.lame)
        self._status = (C.c_double * 16)()
        self._graph = None
        self._key = None
        self._tables = None
        self._rhs_norm = 0.0
        self._amg = _AmgDevice(amg_host(model), dev, True) if precond in _AMG_PRECONDS else None
        self.amg_rebuild = amg_rebuild
        self._tangent = precond == "amg_tangent"
        self._amg_kind = "small_strain"                # what the handle was last set up on ("tangent" / "small_strain")
        self._tangent_setups = self._fallbacks_coarse = self._fallbacks_descent = 0

    def __del__(self):
        _lib.destroy_handle(self, "hfem_cg_destroy")

    # ---- what the forces and the operator depend on besides u_free
    def _state_key(self):
        m = self.model
        ts = [m.node_coords_free, m.node_coords_fixed, m.u_fixed]
        return tuple((None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.dtype)) for t in ts)

    def refresh(self):
        """Coordinates, ``u_fixed`` or the forces changed: re-widen the rows, re-tabulate the forces, redo the AMG numeric
        setup and ``||g(u_free = 0)||``."""
        m, lf, dev = self.model, self.loss_fn, self.device
        with torch.no_grad():
            self._xf.copy_(m.node_coords_free.detach())
            self._xfix.copy_(m.node_coords_fixed.detach())
            self._ufix.copy_(m.u_fixed_rows().detach())
            flags = HFEM_FLAG_NO_GX
            if m.neumann_edges is None or m.N_edges == 0:
                te, tc, flags = None, [0.0] * 4, flags | HFEM_FLAG_NO_EDGES
            else:
                te, tc = lf._traction(_Frozen(m, self._xf, self._xfix), self.t_force)
                te = None if te is None else te.to(device=dev, dtype=F64).contiguous()
            self._tables = (self._body(), te, None if tc is None else (C.c_double * 4)(*tc), flags)
            if self._amg is not None and not self._tangent:
                self._small_strain_setup()
            self._energy(self._zero, self._gz)
            self._rhs_norm = float(torch.linalg.vector_norm(self._gz))
        self._key = self._state_key()

    def _fresh(self):
        if self._key is None or self._key != self._state_key():
            self.refresh()

    def _internal_tables(self):
        """The force tables of the launch with NO forces (zero body table, no edges): ``_energy(u, g, tables)`` then gives the
        internal energy ``Pi_int`` and ``f_int = dPi_int/du_free`` alone (``dynamics.HyperNewmarkSolver``)."""
        body = self._body()
        if body is not None:
            body = type(body)()                             # zero-initialised ctypes array of the same length
        return (body, None, (C.c_double * 4)(), HFEM_FLAG_NO_GX | HFEM_FLAG_NO_EDGES)

    # ---- launches (``_energy(u, g, tables=None)`` is the element's: self._out = {Pi, min J, inverted count} and g = dPi/du_free
    # at u, one launch of the energy kernel + its finish; ``tables``: force tables other than the refresh's)
    def _linearise(self):
        """Bind the driver to ``self._u`` and build the preconditioner there (one diag launch + the info reduction)."""
        check(_lib.lib().hfem_cg_setup_hyper(
            self._h, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(self._u),
            ptr(self._ufix) if self._ufix.numel() else None, self._lame, float(self.loss_fn._W),
            1 if self.precond == "block_jacobi" else 0, ptr(self.diag), ptr(self._info), stream_ptr(self.device)),
            "hfem_cg_setup_hyper")

    def _small_strain_setup(self):
        """The hierarchy of the small-strain operator at the current coordinates (physical convention): ``"amg"``'s numbers."""
        lam, mu = self.loss_fn.lame
        self._amg.setup(self._xf, self._xfix, (C.c_double * 4)(lam + 2 * mu, lam, lam + 2 * mu, mu), float(self.loss_fn._W))
        self._amg_kind = "small_strain"

    def _tangent_setup(self):
        """The hierarchy of K_T at ``self._u``; safeguard (a): the small-strain one when its coarsest matrix is not positive
        definite."""
        self._tangent_setups += 1
        if self._amg.setup_hyper(self._xf, self._xfix, self._u, self._ufix, self._lame, float(self.loss_fn._W)):
            self._amg_kind = "tangent"
        else:
            self._fallbacks_coarse += 1
            self._small_strain_setup()

    def _read_status(self):
        check(_lib.lib().hfem_cg_status(self._h, self._status, stream_ptr(self.device)), "hfem_cg_status")
        return list(self._status)

    def _iterate(self):
        args = (ptr(self._delta), self.iters_per_graph, stream_ptr(self.device))
        if self._amg is None:
            check(_lib.lib().hfem_cg_iterate(self._h, *args), "hfem_cg_iterate")
        else:
            check(_lib.lib().hfem_cg_iterate_amg(self._h, self._amg._h, *args), "hfem_cg_iterate_amg")

    def _replay(self):
        if self._graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                        # captured, not executed
                self._iterate()
            self._graph = g
        self._graph.replay()

    def _precondition(self, r):
        """z = M r on the host's side of the driver: what a CG breakdown at iteration 0 falls back to."""
        if self.precond == "none":
            return r.clone()
        if self._amg is not None:
            z = torch.empty_like(r)
            check(_lib.lib().hfem_amg_vcycle(self._amg._h, ptr(r), ptr(z), stream_ptr(self.device)), "hfem_amg_vcycle")
            return z
        a, b, c = self.diag[:, 0], self.diag[:, 1], self.diag[:, 2]
        det = a * c - b * b
        pd = (a > 0) & (det > 0) & torch.isfinite(det)       # store_jacobi_block's rule
        det = torch.where(pd, det, torch.ones_like(det))
        i00, i01, i11 = torch.where(pd, c / det, torch.ones_like(a)), torch.where(pd, -b / det, torch.zeros_like(a)), \
            torch.where(pd, a / det, torch.ones_like(a))
        return torch.stack([i00 * r[:, 0] + i01 * r[:, 1], i01 * r[:, 0] + i11 * r[:, 1]], dim=1)

    def _pcg(self, eta, max_iter):
        """The driver on K_T d = -self._g from d = 0 to ||r|| <= eta ||g||, into self._delta.  -> (iterations, reason)"""
        self._delta.zero_()
        args = (ptr(self._g), ptr(self._g), float(eta), 0.0, max_iter, stream_ptr(self.device))
        if self._amg is None:
            check(_lib.lib().hfem_cg_start(self._h, *args), "hfem_cg_start")
        else:
            check(_lib.lib().hfem_cg_start_amg(self._h, self._amg._h, *args), "hfem_cg_start_amg")
        st = self._read_status()
        while not st[ST_HALTED] and st[ST_ITER] < max_iter:
            self._replay()
            st = self._read_status()
        return int(st[ST_ITER]), _REASONS.get(int(st[ST_REASON]), "max_iter")

    def _inner(self, eta):
        """self._delta = the truncated-PCG solution of K_T d = -g to the tolerance eta ||g||.  -> (iterations, reason)"""
        its, reason = self._pcg(eta, self.cg_max_iter)
        if reason == "breakdown" and its == 0:
            self._delta.copy_(-self._precondition(self._g))
        return its, reason

    # ---- the solve
    def solve(self) -> NewtonInfo:
        m = self.model
        self._fresh()
        hist: List[dict] = []
        with torch.no_grad():
            self._u.copy_(m.u_free.detach())
            self._linearise()
            min_j, count = self._info.tolist()
            self._energy(self._u, self._g)
            energy = float(self._out[0])
            gn = float(torch.linalg.vector_norm(self._g))
            if count > 0:
                return NewtonInfo(0, 0, gn, self._rhs_norm, energy, min_j, False, "inverted", hist)
            tol = max(self.rtol * self._rhs_norm, self.atol)
            k, cg_total, gn_prev, reason = 0, 0, None, ""
            rebuild = self._tangent                          # amg_rebuild="solve": before the first inner solve only
            while True:
                if gn <= tol:
                    reason = "rtol" if self.rtol * self._rhs_norm >= self.atol else "atol"
                    break
                if k >= self.max_newton:
                    reason = "max_newton"
                    break
                if k > 0:
                    self._linearise()
                eta = self.eta_max if gn_prev is None else min(max(0.9 * (gn / gn_prev) ** 2, 1e-12), self.eta_max)
                if rebuild:
                    self._tangent_setup()
                    rebuild = self.amg_rebuild == "newton"
                its, halt = self._inner(eta)
                gtd = float((self._g * self._delta).sum())
                if self._tangent and self._amg_kind == "tangent" and not gtd < 0.0:
                    self._fallbacks_descent += 1             # safeguard (b): an indefinite cycle gave no descent direction
                    self._small_strain_setup()
                    again, halt = self._inner(eta)
                    its += again
                    gtd = float((self._g * self._delta).sum())
                cg_total += its
                t, accepted = 1.0, False
                for _ in range(self.max_backtracks + 1):
                    torch.add(self._u, self._delta, alpha=t, out=self._trial)
                    self._energy(self._trial, self._gt)
                    e_t, mj_t, _ = self._out.tolist()
                    if math.isfinite(e_t) and e_t <= energy + self.armijo * t * gtd + 4.0 * EPS * abs(energy):
                        accepted = True
                        break
                    t *= 0.5
                hist.append(dict(energy=energy, grad_norm=gn, eta=eta, cg_iterations=its, cg_reason=halt,
                                 step=t if accepted else 0.0, min_J=mj_t if accepted else min_j))
                if self._tangent:
                    hist[-1]["amg"] = self._amg_kind
                if not accepted:
                    reason = "line_search"
                    break
                self._u.copy_(self._trial)
                self._g.copy_(self._gt)
                gn_prev, energy, min_j = gn, e_t, mj_t
                gn = float(torch.linalg.vector_norm(self._g))
                k += 1
            m.u_free.copy_(self._u)                          # rounds once for fp32 models
        return NewtonInfo(k, cg_total, gn, self._rhs_norm, energy, min_j, reason in ("rtol", "atol"), reason, hist)

    # ---- test and measurement helpers
    def apply(self, p: torch.Tensor):
        """Standalone ``q = K_T p`` at the current ``model.u_free`` over the free u rows (fixed rows read as 0) and ``p^T q``
        (0-d device tensor); ``p`` is fp64 ``[n_u, 2]`` in storage order.  Re-linearises (``diag`` and ``info`` follow)."""
        self._fresh()
        with torch.no_grad():
            self._u.copy_(self.model.u_free.detach())
        self._linearise()
        p = _lib.require_gpu_tensor(p.detach(), "p", F64)
        q = torch.empty_like(p)
        pq = torch.empty((), dtype=F64, device=self.device)
        check(_lib.lib().hfem_cg_apply(self._h, ptr(p), ptr(q), ptr(pq), stream_ptr(self.device)), "hfem_cg_apply")
        return q, pq

    def linear_solve(self, b: torch.Tensor, rtol: float, max_iter: Optional[int] = None):
        """``K_T d = b`` at the current ``model.u_free`` by the solver's own PCG from ``d = 0`` to ``||r|| <= rtol ||b||``:
        re-linearises, builds the solver's preconditioner there (``"amg_tangent"``: a tangent setup with safeguard (a)) and
        runs the driver.  ``b`` is fp64 ``[n_u, 2]`` in storage order.  -> ``(d, iterations, reason)``; a breakdown leaves
        ``d`` where the driver stopped."""
        self._fresh()
        b = _lib.require_gpu_tensor(b.detach(), "b", F64)
        with torch.no_grad():
            self._u.copy_(self.model.u_free.detach())
            self._linearise()
            if self._tangent:
                self._tangent_setup()
            torch.neg(b, out=self._g)                        # the driver solves K d = -g0 with g0 = g_zero = -b
            its, reason = self._pcg(rtol, self.cg_max_iter if max_iter is None else int(max_iter))
            return self._delta.clone(), its, reason

    @property
    def amg(self):
        """The AMG hierarchy's report (``_AmgDevice.report``; None without one); with ``precond="amg_tangent"`` also
        ``tangent_setups`` (numeric setups on K_T), ``fallbacks_coarse`` and ``fallbacks_descent`` (safeguards (a), (b))."""
        if self._amg is None:
            return None
        rep = self._amg.report()
        if self._tangent:
            rep.update(tangent_setups=self._tangent_setups, fallbacks_coarse=self._fallbacks_coarse,
                       fallbacks_descent=self._fallbacks_descent, tangent_setup_seconds=self._amg.seconds_hyper)
        return rep

    @property
    def info(self) -> torch.Tensor:
        """``{min J, number of elements with J <= 0}`` of the last linearisation (fp64 device tensor, the same every call)."""
        return self._info


class NewtonKrylovSolver(_NewtonSolverBase):
    """Inexact Newton with truncated PCG for ``model.u_free`` under a ``NeoHookeanLoss2D`` (see the module docstring and
    ``_NewtonSolverBase`` for the arguments and the contract); TRI3 models only, anything else raises ``NotImplementedError``
    (QUAD4 models under a ``Quad4NeoHookeanLoss2D``: ``Quad4NewtonKrylovSolver``)."""

    @staticmethod
    def _check_model(model, loss_fn):
        if not isinstance(loss_fn, NeoHookeanLoss2D):
            raise NotImplementedError("NewtonKrylovSolver: NeoHookeanLoss2D only (an EnergyLoss2D is quadratic in u_free: "
                                      "FrozenMeshSolver / solve_displacement_ solve it in one linear solve)")
        if getattr(model, "nodes_per_element", 3) != 3 or isinstance(loss_fn, Quad4NeoHookeanLoss2D):
            raise NotImplementedError("NewtonKrylovSolver: TRI3 models under a NeoHookeanLoss2D only (QUAD4 models under a "
                                      "Quad4NeoHookeanLoss2D: Quad4NewtonKrylovSolver / quad4_newton_solve_)")

    @staticmethod
    def _make_plan(model, loss_fn):
        from .plan import model_plan
        return model_plan(model, loss_fn.tile_elems, paired=False)

    def _body(self):
        return (C.c_double * 6)(*self.loss_fn._body_table(self.b_force))

    def _energy(self, u, g, tables=None):
        bk, te, tc, flags = self._tables if tables is None else tables
        check(_lib.lib().hfem_tri3_hyper_energy_plan(
            self.plan.handle, 0, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(u),
            ptr(self._ufix) if self._ufix.numel() else None, self._lame, float(self.loss_fn._W), bk, ptr(te), tc,
            self._out.data_ptr(), self._out.data_ptr() + 8, ptr(self._work), None, ptr(g), flags, stream_ptr(self.device)),
            "hfem_tri3_hyper_energy_plan")


class Quad4NewtonKrylovSolver(_NewtonSolverBase):
    """``NewtonKrylovSolver`` for QUAD4 models (``QuadShapeNN2D``) under a ``Quad4NeoHookeanLoss2D``: the same
    arguments, the same contract, the same ``NewtonInfo``.  ``K_T p`` and the block-Jacobi blocks come from
    ``csrc/quad4_hyper_cg.hip`` on the model's own QUAD4 tile plan, residual and energy from the QUAD4 Neo-Hookean energy
    launch on that plan (``hfem_quad4_hyper_energy_plan``; the body force at the 2x2 reference Gauss points, as the loss
    tabulates it), ``precond="amg"`` from the QUAD4 hierarchy of the small-strain operator.  A cell is inverted when
    ``det F <= 0`` at any of its four Gauss points; ``min_J`` is taken over all points.  Anything but a QUAD4 model with a
    ``Quad4NeoHookeanLoss2D`` raises ``NotImplementedError``."""

    @staticmethod
    def _check_model(model, loss_fn):
        if not isinstance(loss_fn, Quad4NeoHookeanLoss2D):
            raise NotImplementedError("Quad4NewtonKrylovSolver: Quad4NeoHookeanLoss2D only (a NeoHookeanLoss2D on a TRI3 model: "
                                      "NewtonKrylovSolver; an EnergyLoss2D is quadratic in u_free: Quad4FrozenMeshSolver / "
                                      "solve_displacement_ solve it in one linear solve)")
        if getattr(model, "nodes_per_element", 3) != 4:
            raise NotImplementedError("Quad4NewtonKrylovSolver: QUAD4 models only (TRI3 models: NewtonKrylovSolver)")

    @staticmethod
    def _make_plan(model, loss_fn):
        return model.tile_plan(loss_fn.tile_elems)

    def _body(self):
        bq = self.loss_fn._quad4_body(self.b_force)
        return None if bq is None else (C.c_double * 8)(*bq)

    def _energy(self, u, g, tables=None):
        bq, te, tc, flags = self._tables if tables is None else tables
        check(_lib.lib().hfem_quad4_hyper_energy_plan(
            self.plan.handle, 0, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(u),
            ptr(self._ufix) if self._ufix.numel() else None, self._lame, bq, ptr(te), tc, self._out.data_ptr(),
            self._out.data_ptr() + 8, ptr(self._work), None, ptr(g), flags, stream_ptr(self.device)),
            "hfem_quad4_hyper_energy_plan")


def assemble_tangent(model, loss_fn) -> torch.Tensor:
    """K_T,ff of the Neo-Hookean energy at the model's current ``u_free`` and coordinates: fp64 ``torch.sparse_bsr_tensor``
    with 2x2 blocks over the free u rows in storage order (Dirichlet columns dropped; ``assemble_stiffness``'s pattern), from
    the AMG tangent assembly kernel (one thread per row, bit-deterministic).  An inverted element or cell contributes zeros:
    exactly the operator ``NewtonKrylovSolver.apply`` applies.  A TRI3 model under a ``NeoHookeanLoss2D`` or a QUAD4 model
    under a ``Quad4NeoHookeanLoss2D``; fp32 models are widened on the way in."""
    quad = getattr(model, "nodes_per_element", 3) == 4
    if not isinstance(loss_fn, NeoHookeanLoss2D) or quad != isinstance(loss_fn, Quad4NeoHookeanLoss2D):
        raise NotImplementedError("assemble_tangent: a TRI3 model under a NeoHookeanLoss2D or a QUAD4 model under a "
                                  "Quad4NeoHookeanLoss2D (the stiffness of an EnergyLoss2D: assemble_stiffness)")
    for name, t in (("node_coords_free", model.node_coords_free), ("u_free", model.u_free)):
        _lib.require_gpu_tensor(t, name, dtype=None)
    dev = model.u_free.device
    host = amg_host(model)
    a = _AmgDevice(host, dev, True)
    rows = lambda t: t.detach().to(F64).contiguous()
    a.assemble_hyper(rows(model.node_coords_free), rows(model.node_coords_fixed), rows(model.u_free), rows(model.u_fixed_rows()),
                     (C.c_double * 2)(*loss_fn.lame), float(loss_fn._W))
    vals = a.values(0, 0).view(-1, 2, 2).clone()
    n = host.levels[0][0]
    i64 = dict(dtype=torch.int64, device=dev)
    crow = torch.as_tensor(host.array(0, 0), **i64)
    col = torch.as_tensor(host.array(0, 1), **i64)
    return torch.sparse_bsr_tensor(crow, col, vals, size=(2 * n, 2 * n))


def newton_solve_(model, loss_fn, **kw) -> NewtonInfo:
    """One-shot ``NewtonKrylovSolver(model, loss_fn, **kw).solve()``: ``model.u_free`` becomes the equilibrium of the
    Neo-Hookean potential at the current coordinates (in place)."""
    return NewtonKrylovSolver(model, loss_fn, **kw).solve()


def quad4_newton_solve_(model, loss_fn, **kw) -> NewtonInfo:
    """One-shot ``Quad4NewtonKrylovSolver(model, loss_fn, **kw).solve()`` for a QUAD4 model under a ``Quad4NeoHookeanLoss2D``."""
    return Quad4NewtonKrylovSolver(model, loss_fn, **kw).solve()
