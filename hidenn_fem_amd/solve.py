"""Frozen-mesh displacement solve: the ``u_free`` that minimises the energy at the model's CURRENT coordinates.

With the nodal coordinates held fixed the HiDeNN-FEM energy is classical P1 finite elements and exactly quadratic in the
displacements, ``E(u) = 1/2 u^T K u - f^T u`` (K symmetric positive definite on the free rows once Dirichlet rows exist), so
its minimum is the linear system ``K_ff u = f - K_fd u_d``.  ``FrozenMeshSolver`` solves it by matrix-free preconditioned
conjugate gradients on the GPU (driver ``csrc/cg.hip``, element kernels ``csrc/tri3_cg.hip``): ``K p`` is the
displacement half of the tuned energy kernel at
``u = p`` with no forces, the residual ``r = -dE/du`` comes from the graded energy kernel itself (so every force table of
``EnergyLoss2D`` -- default traction, a traction or body-force callable, nonzero ``u_fixed`` -- enters with no extra code),
and each iteration is two launches whose scalars (alpha, beta, the stopping test) are reduced on the device.  Iterations run
``iters_per_graph`` at a time as one replayed graph; the host reads one status record per replay.

This is the exact "Step 1" of the alternating scheme of the reference's example 4 (frozen coordinates, optimise ``u_free``),
the fixed-mesh FEM solution to compare an r-adapted energy against, and a warm start for L-BFGS.  Not deterministic: the LDS
atomics of the matrix-vector product make iterates differ in the last bits from run to run (the scalars are reduced in a
fixed order; the deterministic energy path has no solver counterpart).  ``FrozenMeshSolver`` takes TRI3 models; its kernels
run on a paired-slot tile plan (the model's own, or one built for the solver when the planner chose one element per slot for
this mesh).  ``Quad4FrozenMeshSolver`` is the same solver for QUAD4 models (``csrc/quad4_cg.hip``: the matrix-vector product
and the block diagonal for bilinear cells on the model's own QUAD4 plan; the AMG fine level from the four-corner instance of
the assembly kernel of ``csrc/tri3_amg.hip``; the residual from
``hfem_quad4_energy_plan_ex``); everything above the element level -- vector kernels, stopping rule, graph replay, the AMG
hierarchy -- is shared.  ``solve_displacement_`` picks the class by ``model.nodes_per_element``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import require_linear

F64 = torch.float64
HFEM_FLAG_NO_GX = 1
HFEM_FLAG_NO_EDGES = 4
HFEM_FLAG_PHYSICAL_GRAD = 64
_REASONS = {1: "rtol", 2: "atol", 3: "max_iter", 4: "breakdown"}
ST_ITER, ST_RNORM, ST_FNORM, ST_REASON, ST_HALTED = 0, 1, 2, 4, 10     # hfem_cg_status slots (csrc/hfem_amg.h: kIter ...)


@dataclass
class SolveInfo:
    """Outcome of ``FrozenMeshSolver.solve()`` / ``Quad4FrozenMeshSolver.solve()``.
    ``residual_norm``: ||r||_2 over the free u rows of the CG recursion
    (r is updated, not recomputed); ``rhs_norm``: ||f||_2 = ||dE/du|| at ``u_free = 0`` (it includes the ``u_fixed`` term);
    ``reason``: ``"rtol"``, ``"atol"`` (whichever tolerance was the larger one when ||r|| <= max(rtol ||f||, atol)),
    ``"max_iter"`` or ``"breakdown"`` (p^T K p <= 0 or a non-finite scalar: ``u_free`` keeps the last good iterate)."""
    iterations: int
    residual_norm: float
    rhs_norm: float
    converged: bool
    reason: str


class _FrozenSolverBase:
    """What the two element kinds share: argument checks, the solver-owned fp64 working set, the ``refresh`` bookkeeping, the
    PCG loop with its graph replay and status reads, ``apply`` / ``precondition`` / ``amg``.  A subclass says which models it
    takes (``_check_model``), which tile plan the kernels run on (``_make_plan``), the body-force table of its element
    (``_body``) and which graded energy entry point gives ``dE/du`` (``_gradient``)."""

    def __init__(self, model, loss_fn, b_force: Optional[Callable] = None, t_force: Optional[Callable] = None,
                 precond: str = "block_jacobi", rtol: float = 1e-10, atol: float = 0.0, max_iter: Optional[int] = None,
                 iters_per_graph: int = 16):
        self._check_model(model, loss_fn)
        if precond not in ("block_jacobi", "none", "amg"):
            raise ValueError("precond must be 'block_jacobi', 'none' or 'amg'")
        if precond == "amg" and int(model._idx_udir.shape[0]) == 0:
            raise ValueError("precond='amg' needs Dirichlet rows: without them K_ff and the coarse operator are singular")
        if int(iters_per_graph) < 1:
            raise ValueError("iters_per_graph must be >= 1")
        if rtol < 0 or atol < 0:
            raise ValueError("rtol and atol must be >= 0")
        for name, t in (("node_coords_free", model.node_coords_free), ("u_free", model.u_free)):
            _lib.require_gpu_tensor(t, name, dtype=None)
        self.model, self.loss_fn = model, loss_fn
        self.b_force, self.t_force = b_force, t_force
        self.precond, self.rtol, self.atol = precond, float(rtol), float(atol)
        self.iters_per_graph = int(iters_per_graph)
        self.phys = bool(loss_fn._mode_flags(model) & HFEM_FLAG_PHYSICAL_GRAD)
        self.plan = self._make_plan(model, loss_fn)
        dev = model.u_free.device
        self.device = dev
        self.n_u = int(model.u_free.shape[0])
        self.max_iter = max(1000, 4 * self.n_u) if max_iter is None else int(max_iter)
        h = C.c_void_p()
        check(_lib.lib().hfem_cg_create(self.plan.handle, self.n_u, HFEM_FLAG_PHYSICAL_GRAD if self.phys else 0, C.byref(h)),
              "hfem_cg_create")
        self._h = h
        # solver-owned fp64 working set (the captured graph only ever sees these addresses)
        z = dict(dtype=F64, device=dev)
        self._xf = torch.empty(model.node_coords_free.shape, **z)
        self._xfix = torch.empty(model.node_coords_fixed.shape, **z)
        self._ufix = torch.empty((int(model._idx_udir.shape[0]), 2), **z)
        self._u = torch.zeros((self.n_u, 2), **z)
        self._zero = torch.zeros((self.n_u, 2), **z)
        self._g0 = torch.empty((self.n_u, 2), **z)
        self._gz = torch.empty((self.n_u, 2), **z)
        self._loss = torch.empty((), **z)
        self.diag = torch.empty((self.n_u, 3), **z)        # the 2x2 diagonal blocks {K_xx, K_xy, K_yy} of the last refresh
        self._status = (C.c_double * 16)()
        self._graph = None
        self._key = None
        self._tables = None
        self._amg = None
        if precond == "amg":
            self._amg = _AmgDevice(amg_host(model), dev, self.phys)
        self._scale = None            # set_element_scale: an ElementWeights (the operator is K(w)), or None

    def __del__(self):
        _lib.destroy_handle(self, "hfem_cg_destroy")

    def set_element_scale(self, scale: Optional[torch.Tensor]):
        """Solve with ``K(w) = sum_e w_e K_e`` instead of ``K``: ``scale`` is an fp64 ``[ne]`` device tensor of per-element
        stiffness factors in the model's element order (two materials; the SIMP weights of a density design), finite and
        ``> 0`` (``ValueError`` otherwise).  ``None`` restores the homogeneous solve exactly: the same calls as before this
        method existed.  The values are copied; call again after changing them.

        With a scale set the matrix-vector product, the block-Jacobi blocks and the AMG fine level are the ``Scaled``
        instances of the plain kernels (``csrc/tri3_cg.hip`` / ``csrc/quad4_cg.hip``, ``amg_assemble_kernel``), and
        ``solve()`` forms its first residual as ``g0 = g_zero + K(w) u_0`` with one standalone scaled apply instead of the energy launch at ``u_0``.  The Dirichlet
        lift of the homogeneous energy launch would be wrong for ``K(w)``, so a scale requires ``u_fixed == 0``
        (``ValueError`` at the next refresh otherwise).  The energy losses themselves stay homogeneous: ``loss_fn(model)`` and
        the stress recovery do not see the scale."""
        if scale is None:
            self.bind_element_weights(None)
            return
        ne = int(self.model.connectivity.shape[0])
        scale = _lib.require_gpu_tensor(scale.detach(), "scale", F64)
        if tuple(scale.shape) != (ne,):
            raise ValueError(f"set_element_scale: scale must have shape [{ne}] (one factor per element), got {tuple(scale.shape)}")
        if not bool((torch.isfinite(scale) & (scale > 0)).all()):
            raise ValueError("set_element_scale: every factor must be finite and > 0")
        weights = self._scale if self._scale is not None else ElementWeights(self.plan, ne, self.device)
        weights.set(scale)
        self.bind_element_weights(weights)

    def bind_element_weights(self, weights):
        """Make ``weights`` (an ``ElementWeights`` on this solver's plan, or None) the operator's weights: the one place that
        keeps the invalidation rule.  A switch between K and K(w) drops the captured iterations (they hold the other
        operator's kernels); any binding makes the next ``solve`` / ``apply`` / ``relinearise`` refresh."""
        if weights is not None and weights.plan is not self.plan:
            raise ValueError("bind_element_weights: the weights were built on another tile plan")
        if (weights is None) != (self._scale is None):
            self._graph = None
        self._scale = weights
        self._key = None

    def relinearise(self):
        """New values in the bound weight buffers: rebuild the blocks / the AMG values only (one setup), or do the whole
        ``refresh`` when the coordinates, ``u_fixed`` or the binding changed since the last one."""
        if self._key is None or self._key != self._state_key():
            self.refresh()
        else:
            self._setup_operator(self._tables[0])

    def element_energy_inputs(self):
        """What ``ElementWeights.energy`` reads of the last refresh and solve: (fp64 free and fixed coordinate rows, the fp64
        displacement of the last ``solve``, the material table, W, physical convention?)."""
        return self._xf, self._xfix, self._u, self._tables[0], float(self.loss_fn._W), self.phys

    def _setup_operator(self, mat):
        """Bind the operator of this refresh: K, or K(w) once ``set_element_scale`` has given weights."""
        lf, dev = self.loss_fn, self.device
        xfix = ptr(self._xfix) if self._xfix.numel() else None
        pre = 1 if self.precond == "block_jacobi" else 0
        if self._scale is None:
            check(_lib.lib().hfem_cg_setup(self._h, ptr(self._xf), xfix, mat, float(lf._W), pre, ptr(self.diag),
                                           stream_ptr(dev)), "hfem_cg_setup")
            if self._amg is not None:
                self._amg.setup(self._xf, self._xfix, mat, float(lf._W))
            return
        if self._ufix.numel() and bool((self._ufix != 0).any()):
            raise ValueError("set_element_scale needs u_fixed == 0: the Dirichlet lift comes from the homogeneous energy launch")
        check(_lib.lib().hfem_cg_setup_scaled(self._h, ptr(self._xf), xfix, mat, float(lf._W), ptr(self._scale.w_slot), pre,
                                              ptr(self.diag), stream_ptr(dev)), "hfem_cg_setup_scaled")
        if self._amg is not None:
            self._amg.setup_scaled(self._xf, self._xfix, mat, float(lf._W), self._scale.w_elem)

    # ---- what the right-hand side and K depend on
    def _state_key(self):
        m = self.model
        ts = [m.node_coords_free, m.node_coords_fixed, m.u_fixed]
        return tuple((None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.dtype)) for t in ts)

    def refresh(self):
        """Coordinates, ``u_fixed`` or the forces changed: re-widen the coordinate rows, re-tabulate the forces and rebuild
        the preconditioner (one setup launch)."""
        m, lf = self.model, self.loss_fn
        dev = self.device
        with torch.no_grad():
            self._xf.copy_(m.node_coords_free.detach())
            self._xfix.copy_(m.node_coords_fixed.detach())
            self._ufix.copy_(m.u_fixed_rows().detach())
        mat = (C.c_double * 4)(*lf._mat)
        self._setup_operator(mat)
        # force tables exactly as EnergyLoss2D builds them (the coordinates are frozen: a position-dependent traction is a
        # constant table here)
        flags = HFEM_FLAG_NO_GX | (HFEM_FLAG_PHYSICAL_GRAD if self.phys else 0)
        if m.neumann_edges is None or m.N_edges == 0:
            te, tc, flags = None, [0.0] * 4, flags | HFEM_FLAG_NO_EDGES
        else:
            te, tc = lf._traction(_Frozen(m, self._xf, self._xfix), self.t_force)
            te = None if te is None else te.to(device=dev, dtype=F64).contiguous()
        self._tables = (mat, self._body(), te, None if tc is None else (C.c_double * 4)(*tc), flags)
        self._key = self._state_key()

    def _read_status(self):
        check(_lib.lib().hfem_cg_status(self._h, self._status, stream_ptr(self.device)), "hfem_cg_status")
        return list(self._status)

    def _start(self, rtol, atol, max_iter):
        """r = -g0, z = M r, rho, |f| and the stopping rule from ``self._g0`` / ``self._gz``: the record of iteration 0."""
        args = (ptr(self._g0), ptr(self._gz), rtol, atol, max_iter, stream_ptr(self.device))
        if self._amg is None:
            check(_lib.lib().hfem_cg_start(self._h, *args), "hfem_cg_start")
        else:
            check(_lib.lib().hfem_cg_start_amg(self._h, self._amg._h, *args), "hfem_cg_start_amg")

    def _iterate(self):
        """Enqueue ``iters_per_graph`` iterations on ``self._u`` (launches only: capturable)."""
        args = (ptr(self._u), self.iters_per_graph, stream_ptr(self.device))
        if self._amg is None:
            check(_lib.lib().hfem_cg_iterate(self._h, *args), "hfem_cg_iterate")
        else:
            check(_lib.lib().hfem_cg_iterate_amg(self._h, self._amg._h, *args), "hfem_cg_iterate_amg")

    def solve(self) -> SolveInfo:
        m = self.model
        if self._key is None or self._key != self._state_key():
            self.refresh()
        with torch.no_grad():
            self._u.copy_(m.u_free.detach())
            if self._scale is None:
                self._gradient(self._u, self._g0)
                self._gradient(self._zero, self._gz)
            else:                                            # g0 = g_zero + K(w) u_0: the energy launch is homogeneous
                self._gradient(self._zero, self._gz)
                check(_lib.lib().hfem_cg_apply(self._h, ptr(self._u), ptr(self._g0), ptr(self._loss), stream_ptr(self.device)),
                      "hfem_cg_apply")
                self._g0.add_(self._gz)
            self._start(self.rtol, self.atol, self.max_iter)
            st = self._read_status()
            while not st[ST_HALTED] and st[ST_ITER] < self.max_iter:
                self._replay()
                st = self._read_status()
            m.u_free.copy_(self._u)                          # rounds once for fp32 models
        reason = _REASONS.get(int(st[ST_REASON]), "max_iter")
        return SolveInfo(iterations=int(st[ST_ITER]), residual_norm=float(st[ST_RNORM]), rhs_norm=float(st[ST_FNORM]),
                         converged=reason in ("rtol", "atol"), reason=reason)

    def _replay(self):
        if self._graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                        # captured, not executed
                self._iterate()
            self._graph = g
        self._graph.replay()

    def apply(self, p: torch.Tensor):
        """Standalone ``q = K p`` over the free u rows (fixed rows read as 0) and ``p^T q`` (0-d device tensor); ``p`` is fp64
        ``[n_u, 2]`` in storage order.  For tests and measurements."""
        if self._key is None or self._key != self._state_key():
            self.refresh()
        p = _lib.require_gpu_tensor(p.detach(), "p", F64)
        q = torch.empty_like(p)
        pq = torch.empty((), dtype=F64, device=self.device)
        check(_lib.lib().hfem_cg_apply(self._h, ptr(p), ptr(q), ptr(pq), stream_ptr(self.device)), "hfem_cg_apply")
        return q, pq


    @property
    def amg(self):
        """The AMG hierarchy (``precond="amg"``; None otherwise): level count, rows and block nnz per level, operator
        complexity (scalar nnz of all levels over the fine level's), host setup seconds (once per mesh) and the last numeric
        setup seconds (every refresh; device-synchronised)."""
        if self._amg is None:
            return None
        return self._amg.report()

    def precondition(self, r: torch.Tensor):
        """``z = M r`` (one V-cycle, ``precond="amg"`` only) over the free u rows; fp64 ``[n_u, 2]`` in storage order.  For
        tests and measurements."""
        if self._amg is None:
            raise ValueError("precondition(): precond='amg' only")
        if self._key is None or self._key != self._state_key():
            self.refresh()
        r = _lib.require_gpu_tensor(r.detach().contiguous(), "r", F64)
        z = torch.empty_like(r)
        check(_lib.lib().hfem_amg_vcycle(self._amg._h, ptr(r), ptr(z), stream_ptr(self.device)), "hfem_amg_vcycle")
        return z


class FrozenMeshSolver(_FrozenSolverBase):
    """Preconditioned CG for ``model.u_free`` at frozen coordinates (see the module docstring), TRI3 models
    (``Quad4FrozenMeshSolver`` is the QUAD4 one; ``solve_displacement_`` takes either).

    ``b_force`` / ``t_force``: the callables ``loss_fn(model, b_force, t_force)`` would take (default forces when None);
    ``precond``: ``"block_jacobi"`` (2x2 diagonal blocks of K), ``"none"`` or ``"amg"`` (one symmetric V-cycle of smoothed
    aggregation per iteration, ``csrc/tri3_amg.hip``; its host setup is cached on the model, a refresh redoes only the numeric
    setup; needs Dirichlet rows; ``solver.amg`` reports the hierarchy); stopping test
    ``||r||_2 <= max(rtol ||f||_2, atol)``; ``max_iter`` None = ``max(1000, 2 x free dofs)``; ``iters_per_graph``: CG
    iterations per graph replay (iterations behind the one that stopped do nothing on the device).

    ``solve()`` starts from the current ``model.u_free`` (a warm start works), writes the result into it in place and
    returns a ``SolveInfo``.  Nothing else of the model changes: coordinates, ``.grad`` of both parameters, Dirichlet rows.
    ``refresh()`` rebuilds the right-hand side inputs and the preconditioner; ``solve()`` calls it by itself when the
    coordinate rows, ``u_fixed`` or the force inputs changed since the last one (tensor ``_version``).  fp32 models solve
    in fp64 (coordinates widened once per refresh, ``u_free`` rounded once on write-back).  The gradient convention
    follows ``loss_fn`` / ``model`` as the energy does; works in the model's storage row order (``reorder`` any)."""

    @staticmethod
    def _check_model(model, loss_fn):
        require_linear(loss_fn, "FrozenMeshSolver")
        if getattr(model, "nodes_per_element", 3) != 3:
            raise NotImplementedError("FrozenMeshSolver: TRI3 models only (QUAD4 models: Quad4FrozenMeshSolver, or "
                                      "solve_displacement_, which takes either)")
        if getattr(loss_fn, "deterministic", False):
            raise NotImplementedError("FrozenMeshSolver: EnergyLoss2D(deterministic=True) has no solver counterpart "
                                      "(the CG matrix-vector product accumulates with LDS atomics)")

    @staticmethod
    def _make_plan(model, loss_fn):
        plan = _paired_plan(model, loss_fn.tile_elems)
        if not plan.stats["paired"]:
            raise NotImplementedError("FrozenMeshSolver: the CG kernels need a paired-slot tile plan (plan_elem_order 5)")
        return plan

    def _body(self):
        return (C.c_double * 6)(*self.loss_fn._body_table(self.b_force))

    def _gradient(self, u, out):
        """out = dE/du_free at u (fp64 rows), one launch of the graded energy kernel."""
        mat, bk, te, tc, flags = self._tables
        check(_lib.lib().hfem_tri3_energy_plan(
            self.plan.handle, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(u),
            ptr(self._ufix) if self._ufix.numel() else None, mat, float(self.loss_fn._W), bk, ptr(te), tc, 0, -1,
            ptr(self._loss), None, ptr(out), flags, stream_ptr(self.device)), "hfem_tri3_energy_plan")


class Quad4FrozenMeshSolver(_FrozenSolverBase):
    """``FrozenMeshSolver`` for QUAD4 models (``QuadShapeNN2D``): the same arguments, the same contract, the same
    ``SolveInfo``.  ``K p`` and the block-Jacobi blocks come from ``csrc/quad4_cg.hip`` on the model's own QUAD4 tile plan (no
    pairing), the AMG fine level from the four-corner instance of ``csrc/tri3_amg.hip``'s assembly kernel; the residual and ``||f||`` from the graded QUAD4 energy kernel on fp64 rows
    (``hfem_quad4_energy_plan_ex``), so default forces, a body-force callable (evaluated at the 2x2 reference Gauss points, as
    ``EnergyLoss2D`` does), a traction callable and nonzero ``u_fixed`` enter with no solver code of their own.  fp32 models
    solve in fp64 (rows widened per refresh, ``u_free`` rounded once on write-back).  Refuses TRI3 models,
    ``EnergyLoss2D(deterministic=True)`` and the planless cross-check path (``loss_fn.quad4_planless``)."""

    @staticmethod
    def _check_model(model, loss_fn):
        require_linear(loss_fn, "Quad4FrozenMeshSolver")
        if getattr(model, "nodes_per_element", 3) != 4:
            raise NotImplementedError("Quad4FrozenMeshSolver: QUAD4 models only (TRI3 models: FrozenMeshSolver)")
        if getattr(loss_fn, "deterministic", False):
            raise NotImplementedError("Quad4FrozenMeshSolver: EnergyLoss2D(deterministic=True) has no solver counterpart "
                                      "(the CG matrix-vector product accumulates with LDS atomics)")
        if getattr(loss_fn, "quad4_planless", False):
            raise NotImplementedError("Quad4FrozenMeshSolver: quad4_planless=True has no solver counterpart (the CG kernels run "
                                      "on the tile plan)")

    @staticmethod
    def _make_plan(model, loss_fn):
        return model.tile_plan(loss_fn.tile_elems)

    def _body(self):
        bq = self.loss_fn._quad4_body(self.b_force)
        return None if bq is None else (C.c_double * 8)(*bq)

    def _gradient(self, u, out):
        """out = dE/du_free at u (fp64 rows), one launch of the graded QUAD4 energy kernel."""
        mat, bq, te, tc, flags = self._tables
        check(_lib.lib().hfem_quad4_energy_plan_ex(
            self.plan.handle, 0, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(u),
            ptr(self._ufix) if self._ufix.numel() else None, mat, bq, ptr(te), tc, 0, -1, ptr(self._loss), None, ptr(out),
            flags, stream_ptr(self.device)), "hfem_quad4_energy_plan_ex")


class AmgHost:
    """Host setup of the AMG hierarchy of one mesh (``csrc/amg.cpp``; TRI3 or QUAD4 by the connectivity's width): block
    pattern, element fan, aggregation and symbolic products of every level.  Depends on the connectivity, the Dirichlet mask and the u row order only (``amg_host``)."""

    def __init__(self, model):
        conn = np.ascontiguousarray(model.connectivity.detach().cpu().numpy(), dtype=np.int32)
        xs = np.ascontiguousarray(model._x_src, dtype=np.int32)
        us = np.ascontiguousarray(model._u_src, dtype=np.int32)
        h = C.c_void_p()
        check(_lib.lib().hfem_amg_host_create_ex(conn.ctypes.data, conn.shape[0], conn.shape[1], xs.shape[0], xs.ctypes.data,
                                                 us.ctypes.data, C.byref(h)), "hfem_amg_host_create_ex")
        self._h = h
        top = self.info(-1)
        self.seconds = top[4] * 1e-9
        self.levels = [self.info(lvl) for lvl in range(top[0])]

    def __del__(self):
        _lib.destroy_handle(self, "hfem_amg_host_destroy")

    def info(self, level):
        out = (C.c_int64 * 8)()
        check(_lib.lib().hfem_amg_host_info(self._h, level, out), "hfem_amg_host_info")
        return list(out)

    def array(self, level, which):
        n = C.c_int64()
        check(_lib.lib().hfem_amg_host_copy(self._h, level, which, None, C.byref(n)), "hfem_amg_host_copy")
        out = np.empty(n.value, dtype=np.int32)
        check(_lib.lib().hfem_amg_host_copy(self._h, level, which, out.ctypes.data, C.byref(n)), "hfem_amg_host_copy")
        return out


def amg_host(model) -> AmgHost:
    """The model's AMG host setup, built on first use and cached beside its tile plans (topology, Dirichlet mask and row order
    never change for a model)."""
    key = ("amg_host",)
    if key not in model._plans:
        model._plans[key] = AmgHost(model)
    return model._plans[key]


class _AmgDevice:
    """Device hierarchy of an ``AmgHost`` (``csrc/tri3_amg.hip``) with the dense coarsest matrix and its inverse (formed by
    ``torch.linalg`` at setup: not on the cycle's path)."""

    def __init__(self, host, device, phys):
        self.host, self.device = host, device
        h = C.c_void_p()
        check(_lib.lib().hfem_amg_create(_lib.dev_index(device), host._h, HFEM_FLAG_PHYSICAL_GRAD if phys else 0, C.byref(h)),
              "hfem_amg_create")
        self._h = h
        n, bs = host.levels[-1][:2]
        self.coarse = torch.empty((n * bs, n * bs), dtype=F64, device=device)
        self.coarse_inv = torch.empty_like(self.coarse)
        self.setups, self.seconds = 0, 0.0
        self.setups_hyper, self.seconds_hyper = 0, 0.0   # setup_hyper: the tangent hierarchy on the same handle

    def __del__(self):
        _lib.destroy_handle(self, "hfem_amg_destroy")

    def assemble(self, xf, xfix, mat, W):
        check(_lib.lib().hfem_amg_assemble(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, mat, W,
                                           stream_ptr(self.device)), "hfem_amg_assemble")

    def setup(self, xf, xfix, mat, W):
        import time
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        check(_lib.lib().hfem_amg_setup(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, mat, W, ptr(self.coarse),
                                        stream_ptr(self.device)), "hfem_amg_setup")
        inv = torch.linalg.inv(self.coarse)
        self.coarse_inv.copy_(0.5 * (inv + inv.T))
        check(_lib.lib().hfem_amg_set_coarse(self._h, ptr(self.coarse_inv)), "hfem_amg_set_coarse")
        torch.cuda.synchronize(self.device)
        self.seconds = time.perf_counter() - t0
        self.setups += 1

    def assemble_shifted(self, xf, xfix, mat, W, c_k, c_m, lumped):
        """Level-0 A values = c_k K_ff + c_m M_ff (implicit dynamics; ``c_m`` includes the density)."""
        check(_lib.lib().hfem_amg_assemble_shifted(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, mat, W, float(c_k),
                                                   float(c_m), 1 if lumped else 0, stream_ptr(self.device)),
              "hfem_amg_assemble_shifted")

    def setup_shifted(self, xf, xfix, mat, W, c_k, c_m, lumped):
        """``setup`` on the assembled shifted operator ``c_k K_ff + c_m M_ff`` (SPD: the coarse inverse as in ``setup``)."""
        import time
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        check(_lib.lib().hfem_amg_setup_shifted(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, mat, W, float(c_k),
                                                float(c_m), 1 if lumped else 0, ptr(self.coarse), stream_ptr(self.device)),
              "hfem_amg_setup_shifted")
        inv = torch.linalg.inv(self.coarse)
        self.coarse_inv.copy_(0.5 * (inv + inv.T))
        check(_lib.lib().hfem_amg_set_coarse(self._h, ptr(self.coarse_inv)), "hfem_amg_set_coarse")
        torch.cuda.synchronize(self.device)
        self.seconds = time.perf_counter() - t0
        self.setups += 1

    def assemble_scaled(self, xf, xfix, mat, W, w_elem):
        """Level-0 A values = K(w)_ff = sum_e w_e K_e,ff; ``w_elem`` fp64 ``[ne]`` by element id."""
        check(_lib.lib().hfem_amg_assemble_scaled(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, mat, W, ptr(w_elem),
                                                  stream_ptr(self.device)), "hfem_amg_assemble_scaled")

    def setup_scaled(self, xf, xfix, mat, W, w_elem):
        """``setup`` on the assembled ``K(w)_ff`` (SPD for w > 0: the coarse inverse as in ``setup``)."""
        import time
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        check(_lib.lib().hfem_amg_setup_scaled(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, mat, W, ptr(w_elem),
                                               ptr(self.coarse), stream_ptr(self.device)), "hfem_amg_setup_scaled")
        inv = torch.linalg.inv(self.coarse)
        self.coarse_inv.copy_(0.5 * (inv + inv.T))
        check(_lib.lib().hfem_amg_set_coarse(self._h, ptr(self.coarse_inv)), "hfem_amg_set_coarse")
        torch.cuda.synchronize(self.device)
        self.seconds = time.perf_counter() - t0
        self.setups += 1

    def assemble_hyper(self, xf, xfix, u, ufix, lame, W):
        """Level-0 A values = the Neo-Hookean tangent K_T,ff at the coordinates and the displacement rows."""
        check(_lib.lib().hfem_amg_assemble_hyper(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, ptr(u),
                                                 ptr(ufix) if ufix.numel() else None, lame, W, stream_ptr(self.device)),
              "hfem_amg_assemble_hyper")

    def setup_hyper(self, xf, xfix, u, ufix, lame, W) -> bool:
        """``setup`` on the assembled Neo-Hookean tangent at ``u`` with the near-null space at the deformed position.  K_T can
        be indefinite: the symmetrised coarsest matrix is Cholesky-factored, and when that fails (K_T has a non-positive
        direction in the coarse space) no coarse inverse is bound and False is returned -- the caller sets the handle up again
        (``setup``) before the next cycle."""
        import time
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        check(_lib.lib().hfem_amg_setup_hyper(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, ptr(u),
                                              ptr(ufix) if ufix.numel() else None, lame, W, ptr(self.coarse),
                                              stream_ptr(self.device)), "hfem_amg_setup_hyper")
        sym = 0.5 * (self.coarse + self.coarse.T)
        ok = bool(torch.isfinite(sym).all())
        if ok:
            chol, info = torch.linalg.cholesky_ex(sym)
            ok = int(info) == 0
        if ok:
            inv = torch.cholesky_inverse(chol)
            self.coarse_inv.copy_(0.5 * (inv + inv.T))
            check(_lib.lib().hfem_amg_set_coarse(self._h, ptr(self.coarse_inv)), "hfem_amg_set_coarse")
        torch.cuda.synchronize(self.device)
        self.seconds_hyper = time.perf_counter() - t0
        self.setups_hyper += 1
        return ok

    def values(self, level, which):
        """Device fp64 array ``which`` of a level (hfem_amg_values: 0 A blocks, 1 D^-1, 2 coefficients, 3 near-null space,
        4 P_tent, 5 P blocks)."""
        n = C.c_int64()
        check(_lib.lib().hfem_amg_values(self._h, level, which, None, C.byref(n), None), "hfem_amg_values")
        out = torch.empty(n.value, dtype=F64, device=self.device)
        check(_lib.lib().hfem_amg_values(self._h, level, which, ptr(out), C.byref(n), stream_ptr(self.device)),
              "hfem_amg_values")
        return out

    def report(self):
        lv = self.host.levels
        nnz = [L[2] * L[1] * L[1] for L in lv]
        return dict(levels=len(lv), rows=[L[0] * L[1] for L in lv], block_rows=[L[0] for L in lv],
                    block_nnz=[L[2] for L in lv], block_size=[L[1] for L in lv],
                    operator_complexity=sum(nnz) / nnz[0], host_setup_seconds=self.host.seconds,
                    numeric_setup_seconds=self.seconds, numeric_setups=self.setups)


class ElementWeights:
    """Per-element weights of ``K(w)`` on one tile plan (``csrc/topopt.hip``, ``hfem_topt``): ``w_elem`` fp64 ``[ne]`` by
    element id (what the AMG assembly reads) and ``w_slot``, the same weights once per slot of the plan in the order of its
    element records (what the scaled apply and diag kernels read; entries without an element 0).  Both buffers are
    allocated once, so the pointer a solver bound stays valid across ``set`` / ``simp``.  ``centroids`` / ``volumes`` (fp64
    ``[ne, 2]`` / ``[ne]``, any device) and ``radius > 0`` add the linear density filter (``filter``)."""

    def __init__(self, plan, ne, device, centroids=None, volumes=None, radius=0.0):
        self.plan, self.ne, self.device = plan, int(ne), device
        h = C.c_void_p()
        c = v = None
        if volumes is not None:                                  # the volume constraint of ``oc`` needs them, filter or not
            v = np.ascontiguousarray(volumes.detach().cpu().numpy(), dtype=np.float64)
        if radius > 0:
            c = np.ascontiguousarray(centroids.detach().cpu().numpy(), dtype=np.float64)
            if c.shape != (self.ne, 2) or v is None or v.shape != (self.ne,):
                raise ValueError("ElementWeights: centroids must be [ne, 2] and volumes [ne]")
        check(_lib.lib().hfem_topt_create(plan.handle, None if c is None else c.ctypes.data, None if v is None else v.ctypes.data,
                                          self.ne, float(radius), C.byref(h)), "hfem_topt_create")
        self._h = h
        n = int(_lib.lib().hfem_topt_slots(h))
        self.w_elem = torch.ones(self.ne, dtype=F64, device=device)
        self.w_slot = torch.zeros(n, dtype=F64, device=device)

    def __del__(self):
        _lib.destroy_handle(self, "hfem_topt_destroy")

    def simp(self, rho, penal, e_min):
        """``w_e = e_min + rho_e^penal (1 - e_min)`` into both buffers (one launch)."""
        rho = _lib.require_gpu_tensor(rho, "rho", F64)
        check(_lib.lib().hfem_topt_weights(self._h, ptr(rho), float(penal), float(e_min), ptr(self.w_elem), ptr(self.w_slot),
                                           stream_ptr(self.device)), "hfem_topt_weights")

    def set(self, w):
        """The weights themselves (``penal = 1``, ``e_min = 0`` passes them through bit for bit)."""
        self.simp(w, 1.0, 0.0)

    def filter(self, x, transpose=False):
        """``F x`` or ``F^T x`` of the density filter (the identity without a radius); fp64 ``[ne]``."""
        x = _lib.require_gpu_tensor(x, "x", F64)
        out = torch.empty_like(x)
        check(_lib.lib().hfem_topt_filter(self._h, ptr(x), ptr(out), 1 if transpose else 0, stream_ptr(self.device)),
              "hfem_topt_filter")
        return out

    def energy(self, xf, xfix, u, mat, W, phys, rho_f, penal, e_min, ce, dc):
        """``ce[e] = u_e^T K_e u_e`` (unscaled) and ``dc[e] = -penal rho_f[e]^(penal-1) (1 - e_min) ce[e]``: one launch."""
        check(_lib.lib().hfem_topt_energy(self._h, ptr(xf), ptr(xfix) if xfix.numel() else None, ptr(u), mat, float(W),
                                          HFEM_FLAG_PHYSICAL_GRAD if phys else 0, ptr(rho_f), float(penal), float(e_min), ptr(ce),
                                          ptr(dc), stream_ptr(self.device)), "hfem_topt_energy")

    def oc(self, rho, dc, dv, vol_target, move, n_bisect, rho_new, rho_f_new):
        """The optimality-criteria update (launches only: capturable)."""
        check(_lib.lib().hfem_topt_oc(self._h, ptr(rho), ptr(dc), ptr(dv), float(vol_target), float(move), int(n_bisect),
                                      ptr(rho_new), ptr(rho_f_new), stream_ptr(self.device)), "hfem_topt_oc")

    def status(self):
        """``hfem_topt_status`` of the last update: dict of lambda_lo, lambda_hi, volume (at lambda_hi), steps, feasible."""
        st = (C.c_double * 16)()
        check(_lib.lib().hfem_topt_status(self._h, st, stream_ptr(self.device)), "hfem_topt_status")
        return dict(lambda_lo=st[0], lambda_hi=st[1], volume=st[2], steps=int(st[3]), feasible=bool(st[4]))


def assemble_stiffness(model, loss_fn, elem_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K_ff of the model at its current coordinates: fp64 ``torch.sparse_bsr_tensor`` with 2x2 blocks over the free u rows in
    storage order (Dirichlet columns dropped), from the AMG assembly kernel (one thread per row, deterministic).  The gradient
    convention follows ``loss_fn`` / ``model`` as the energy does.  TRI3 and QUAD4 models.  ``elem_scale`` (fp64 ``[ne]``
    device tensor, the model's element order): ``K(w)_ff = sum_e w_e K_e,ff`` instead."""
    require_linear(loss_fn, "assemble_stiffness")
    _lib.require_gpu_tensor(model.node_coords_free, "node_coords_free", dtype=None)
    dev = model.u_free.device
    phys = bool(loss_fn._mode_flags(model) & HFEM_FLAG_PHYSICAL_GRAD)
    host = amg_host(model)
    a = _AmgDevice(host, dev, phys)
    xf = model.node_coords_free.detach().to(F64).contiguous()
    xfix = model.node_coords_fixed.detach().to(F64).contiguous()
    if elem_scale is None:
        a.assemble(xf, xfix, (C.c_double * 4)(*loss_fn._mat), float(loss_fn._W))
    else:
        w = _lib.require_gpu_tensor(elem_scale.detach(), "elem_scale", F64)
        if tuple(w.shape) != (int(model.connectivity.shape[0]),):
            raise ValueError("assemble_stiffness: elem_scale must hold one factor per element")
        a.assemble_scaled(xf, xfix, (C.c_double * 4)(*loss_fn._mat), float(loss_fn._W), w)
    vals = a.values(0, 0).view(-1, 2, 2).clone()
    n = host.levels[0][0]
    i64 = dict(dtype=torch.int64, device=dev)
    crow = torch.as_tensor(host.array(0, 0), **i64)
    col = torch.as_tensor(host.array(0, 1), **i64)
    return torch.sparse_bsr_tensor(crow, col, vals, size=(2 * n, 2 * n))


def _paired_plan(model, tile_elems):
    """The model's tile plan when it has paired slots, else a paired plan of the same mesh and row maps (cached on the model
    beside its own plans).  The planner's auto policy gives meshes with few fan-adjacent partners -- zigzag splits such as
    example 4's plate, Delaunay meshes -- the one-element-per-slot order; the CG kernels exist for paired plans only, where an
    element without a partner is simply a slot with one element."""
    from .plan import model_plan
    return model_plan(model, tile_elems, paired=True)


class _Frozen:
    """What ``EnergyLoss2D._traction`` reads of a model (``nm_edges``), over the solver's fp64 coordinate rows."""

    def __init__(self, model, xf, xfix):
        self._m, self._xf, self._xfix = model, xf, xfix

    @property
    def nm_edges(self):
        from . import ops
        m = self._m
        coords = ops.AssembleRowsFn.apply(self._xf, self._xfix, m._idx_free, m._idx_fixed, m.Nnodes)
        from .models import NeumannEdgesWrapper
        return NeumannEdgesWrapper(coords, m.neumann_edges)


def solve_displacement_(model, loss_fn, **kw) -> SolveInfo:
    """One-shot ``FrozenMeshSolver(model, loss_fn, **kw).solve()`` -- ``Quad4FrozenMeshSolver`` for a QUAD4 model:
    ``model.u_free`` minimises the energy at the current coordinates (in place)."""
    cls = Quad4FrozenMeshSolver if getattr(model, "nodes_per_element", 3) == 4 else FrozenMeshSolver
    return cls(model, loss_fn, **kw).solve()
