"""Implicit transient dynamics of a TRI3 or QUAD4 model: Newmark time stepping on the operator ``A = c_M M + c_K K``.

The semi-discrete system over the free ``u`` rows is ``M u'' + C u' + K u = load(t) b0`` with ``K`` the operator the frozen-mesh
solver applies at the model's CURRENT coordinates (``hfem_cg_apply``), ``M`` the consistent or lumped mass of
``hfem_mass_apply`` (density rho), ``C = alpha_R M + beta_R K`` (Rayleigh damping) and ``b0 = -dE/du(u_free = 0)``, the vector
``FrozenMeshSolver`` forms as ``g_zero``: forces and the ``u_fixed`` term together, both scaled by the host callable
``load(t)``.  Dirichlet values are constant in time.  Per step with ``(beta, gamma, dt)``, in the a-form::

    u~ = u + dt v + dt^2 (1/2 - beta) a        v~ = v + dt (1 - gamma) a        w = u~ + beta_R v~
    A a+ = load(t + dt) b0 - K w - alpha_R M v~,   A = c_M M + c_K K,  c_M = 1 + gamma dt alpha_R,  c_K = beta dt^2 + gamma dt beta_R
    u+ = u~ + beta dt^2 a+                     v+ = v~ + gamma dt a+

The solve is the PCG driver of the frozen-mesh solve (``csrc/cg.hip``) on the ``MASS`` instances of its plain element kernels
(``csrc/tri3_cg.hip``, ``csrc/quad4_cg.hip``: the mass term is formed inside the slot loop of the ``K`` apply, with no second pass of gathers),
warm-started from the previous ``a``, preconditioned by a smoothed-aggregation hierarchy built on ``A`` itself
(``hfem_amg_setup_shifted``), the 2x2 diagonal blocks of ``A``, or nothing; the three vector passes of a step are
``csrc/dynamics.hip``.  The initial acceleration solves ``M a0 = load(0) b0 - K u0 - C v0`` (``c_K = 0``).  With a lumped mass
and ``c_K = 0`` -- that solve, and every step of explicit central difference (``beta = 0``, ``beta_R = 0``) -- ``A`` is block
diagonal and the stored inverse blocks are applied once instead of CG (``StepInfo.iterations == 0``).

``2 beta >= gamma >= 1/2`` is the unconditional-stability condition; it is documented, not enforced (``beta = 0`` is the
conditionally stable explicit scheme).  No reference counterpart: the reference has no mass matrix.

``HyperNewmarkSolver`` is the same scheme at finite strain: ``M u'' + alpha_R M u' + f_int(u) = load(t) b_ext`` with
``f_int`` the gradient of the Neo-Hookean internal energy, one Newton-Krylov solve per step on ``A(u) = c_M M + c_K K_T(u)`` (the
``MASS`` instances of the tangent kernels, ``csrc/tri3_hyper_cg.hip``, ``csrc/quad4_hyper_cg.hip``).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D, require_linear
from .modal import GRAM_PARTIALS, _frozen_class
from .post import node_adjacency
from .solve import (_AmgDevice, _REASONS, amg_host, HFEM_FLAG_PHYSICAL_GRAD, ST_FNORM, ST_HALTED, ST_ITER, ST_REASON,
                    ST_RNORM)

F64 = torch.float64


@dataclass
class StepInfo:
    """Outcome of one time step: ``SolveInfo``'s fields for the step's linear solve plus ``t``, the time the step arrived at.
    ``reason`` is ``"direct"`` (with ``iterations == 0``) when ``A`` was block diagonal and no CG ran."""
    t: float
    iterations: int
    residual_norm: float
    rhs_norm: float
    converged: bool
    reason: str


class _MassOperator:
    """``hfem_mass_apply`` on one model: the adjacency and row arrays it takes, and the fp64 coordinates by node id
    (``refresh()`` re-reads them).  ``apply(p, q)``: ``q = rho M p`` over the free u rows, one column."""

    def __init__(self, model, npe, device, n_u, density, lumped):
        self.model, self.npe, self.device, self.n_u, self.density, self.lumped = model, npe, device, n_u, density, lumped
        adj_ptr, adj = node_adjacency(model._conn32, model.Nnodes)
        self._adj_ptr, self._adj = adj_ptr.to(device), adj.to(device)
        self._row_node = model._idx_ufree.to(device=device, dtype=torch.int32).contiguous()
        node_row = torch.full((model.Nnodes,), -1, dtype=torch.int32, device=device)
        node_row[self._row_node.long()] = torch.arange(n_u, dtype=torch.int32, device=device)
        self._node_row = node_row
        self._x64 = None

    def refresh(self):
        self._x64 = self.model.coords.detach().to(F64).contiguous()

    def apply(self, p, q):
        md = self.model
        check(_lib.lib().hfem_mass_apply(_lib.dev_index(self.device), self.npe, ptr(self._x64), ptr(md._conn32), md.Nelems,
                                         md.Nnodes, ptr(self._adj_ptr), ptr(self._adj), ptr(self._row_node), ptr(self._node_row),
                                         self.n_u, self.density, 1 if self.lumped else 0, ptr(p), 1, ptr(q),
                                         stream_ptr(self.device)), "hfem_mass_apply")


def _check_newmark(dt, beta, gamma, density, mass, precond, iters_per_graph, rtol, atol, rayleigh):
    """The argument checks both time steppers share.  -> (dt, beta, gamma, density, alpha_R, beta_R) as floats"""
    if mass not in ("consistent", "lumped"):
        raise ValueError("mass must be 'consistent' or 'lumped'")
    if precond not in ("amg", "block_jacobi", "none"):
        raise ValueError("precond must be 'amg', 'block_jacobi' or 'none'")
    dt, beta, gamma, density = float(dt), float(beta), float(gamma), float(density)
    alpha_r, beta_r = (float(c) for c in rayleigh)
    if not dt > 0.0:
        raise ValueError("dt must be > 0")
    if not beta >= 0.0:
        raise ValueError("beta must be >= 0")
    if not gamma >= 0.5:
        raise ValueError("gamma must be >= 1/2")
    if not (alpha_r >= 0.0 and beta_r >= 0.0):
        raise ValueError("the Rayleigh coefficients (alpha_R, beta_R) must be >= 0")
    if not density > 0.0:
        raise ValueError("density must be > 0")
    if int(iters_per_graph) < 1:
        raise ValueError("iters_per_graph must be >= 1")
    if rtol < 0 or atol < 0:
        raise ValueError("rtol and atol must be >= 0")
    return dt, beta, gamma, density, alpha_r, beta_r


class NewmarkSolver:
    """Newmark time stepping for a TRI3 or QUAD4 mesh model with an ``EnergyLoss2D`` (see the module docstring).

    ``dt`` > 0; ``density`` > 0; ``mass``: ``"consistent"`` or ``"lumped"``; ``beta`` >= 0, ``gamma`` >= 1/2; ``rayleigh`` =
    ``(alpha_R, beta_R)``, both >= 0; ``load``: host callable ``t -> float`` (default: constant 1); ``precond``: ``"amg"`` (a
    hierarchy on ``A``; needs Dirichlet rows and ``c_K > 0``), ``"block_jacobi"`` or ``"none"``; ``rtol``, ``atol``,
    ``max_iter`` (None = ``max(1000, 4 x free rows)``) and ``iters_per_graph`` as ``FrozenMeshSolver``; ``b_force`` /
    ``t_force``: the callables ``loss_fn(model, b_force, t_force)`` would take.

    ``set_state(u, v)`` sets the initial displacement and velocity (fp64 ``[n_u, 2]`` in storage order; default
    ``model.u_free`` and 0), solves for ``a0`` and resets ``t`` to 0; the first ``step()`` calls it when nobody has.
    ``step(n)`` advances ``n`` steps and returns their ``StepInfo``; ``.t``, ``.u``, ``.v``, ``.a`` are the current state (fp64
    device tensors).  ``model.u_free`` receives ``u`` at the end of every ``step()`` call (fp32 models are stepped in fp64 and
    rounded once there); nothing else of the model changes.  ``step()`` refreshes by the frozen solver's state key when the
    coordinate rows or ``u_fixed`` moved (``refresh()`` by hand after the force callables changed): ``u, v, a`` are kept, ``K``,
    ``M``, ``b0``, ``A`` and its preconditioner are rebuilt.

    It owns a ``FrozenMeshSolver`` / ``Quad4FrozenMeshSolver`` (plain ``K w``, ``b0``, the refresh bookkeeping and the force
    tables) and a second PCG handle on the same tile plan, set up shifted.  Refuses non-linear losses,
    ``EnergyLoss2D(deterministic=True)`` and CPU models.  Not bitwise reproducible: the apply's LDS atomics carry last-bit noise.

    THE NUMBERS ARE PHYSICAL ONLY WITH ``grad_convention="physical"`` (as ``ModalSolver``).  ``K`` and ``b0`` are those of the
    energy ``loss_fn`` computes, so a TRI3 loss with the default ``gauss_order=4`` carries the reference's factor 1/2 on both."""

    def __init__(self, model, loss_fn, dt: float, density: float = 1.0, mass: str = "consistent", beta: float = 0.25,
                 gamma: float = 0.5, rayleigh=(0.0, 0.0), load: Optional[Callable] = None, precond: str = "amg",
                 rtol: float = 1e-10, atol: float = 0.0, max_iter: Optional[int] = None, iters_per_graph: int = 16,
                 b_force: Optional[Callable] = None, t_force: Optional[Callable] = None):
        require_linear(loss_fn, "NewmarkSolver")
        npe = getattr(model, "nodes_per_element", 3)
        if npe not in (3, 4) or not hasattr(model, "_conn32"):
            raise NotImplementedError("NewmarkSolver: TRI3 and QUAD4 mesh models")
        dt, beta, gamma, density, alpha_r, beta_r = _check_newmark(dt, beta, gamma, density, mass, precond, iters_per_graph, rtol,
                                                                   atol, rayleigh)
        c_k = beta * dt * dt + gamma * dt * beta_r
        c_m = 1.0 + gamma * dt * alpha_r
        if precond == "amg" and int(model._idx_udir.shape[0]) == 0:
            raise ValueError("precond='amg' needs Dirichlet rows (rigid-body modes are out of scope)")
        if precond == "amg" and c_k == 0.0:
            raise ValueError("precond='amg' with c_K = beta dt^2 + gamma dt beta_R = 0: A is a pure mass matrix and needs no "
                             "hierarchy (use 'block_jacobi')")
        cls = _frozen_class(npe)
        # refuses deterministic=True and a CPU model: there is no CPU fallback
        self.solver = cls(model, loss_fn, b_force=b_force, t_force=t_force, precond="none")
        self.model, self.loss_fn, self.npe = model, loss_fn, npe
        self.dt, self.density, self.mass, self.beta, self.gamma = dt, density, mass, beta, gamma
        self.alpha_r, self.beta_r, self.c_k, self.c_m = alpha_r, beta_r, c_k, c_m
        self.load = (lambda t: 1.0) if load is None else load
        self.precond, self.rtol, self.atol = precond, float(rtol), float(atol)
        self.iters_per_graph = int(iters_per_graph)
        self.lumped = mass == "lumped"
        self.device = dev = self.solver.device
        self.phys = self.solver.phys
        self.n_u = n_u = self.solver.n_u
        self.len = 2 * n_u
        self.max_iter = max(1000, 4 * n_u) if max_iter is None else int(max_iter)
        h = C.c_void_p()
        check(_lib.lib().hfem_cg_create(self.solver.plan.handle, n_u, HFEM_FLAG_PHYSICAL_GRAD if self.phys else 0, C.byref(h)),
              "hfem_cg_create")
        self._h = h
        self._amg = _AmgDevice(amg_host(model), dev, self.phys) if precond == "amg" else None
        self._mass = _MassOperator(model, npe, dev, n_u, density, self.lumped)
        z = dict(dtype=F64, device=dev)
        new = lambda: torch.zeros((n_u, 2), **z)
        self.u, self.v, self.a = new(), new(), new()
        self._ut, self._vt, self._w, self._kw, self._mv, self._aa = new(), new(), new(), new(), new(), new()
        self._g0, self._gz, self._b0 = new(), new(), new()
        self.diag = torch.empty((n_u, 3), **z)            # the 2x2 diagonal blocks {A_xx, A_xy, A_yy} of the last setup
        self._pq = torch.empty((), **z)
        self._stack = torch.zeros((6, n_u, 2), **z)       # energy(): [v, u, u | M v, K u, b0]
        self._gram = torch.zeros(9, **z)
        self._gram_partials = torch.empty(GRAM_PARTIALS, **z)
        self._status = (C.c_double * 16)()
        self._graphs = {}
        self._bound = None                                # (c_k, c_m) the shifted handle is set up with
        self._key = None
        self._started = False
        self.t = 0.0

    def __del__(self):
        _lib.destroy_handle(self, "hfem_cg_destroy")

    # ---- operators
    def _mat(self):
        return (C.c_double * 4)(*self.loss_fn._mat), float(self.loss_fn._W)

    def _bind(self, c_k, c_m):
        """Set the shifted handle up for ``c_k K + c_m rho M`` (block diagonal always stored: the direct path reads it)."""
        s = self.solver
        mat, W = self._mat()
        check(_lib.lib().hfem_cg_setup_shifted(self._h, ptr(s._xf), ptr(s._xfix) if s._xfix.numel() else None, mat, W, c_k,
                                               c_m * self.density, 1 if self.lumped else 0,
                                               1 if self.precond in ("block_jacobi", "amg") else 0, ptr(self.diag),
                                               stream_ptr(self.device)), "hfem_cg_setup_shifted")
        self._bound = (c_k, c_m)

    def _bind_step(self):
        self._bind(self.c_k, self.c_m)
        if self._amg is not None:
            s = self.solver
            mat, W = self._mat()
            self._amg.setup_shifted(s._xf, s._xfix, mat, W, self.c_k, self.c_m * self.density, self.lumped)

    def refresh(self):
        """Coordinates, ``u_fixed`` or the forces changed: the frozen solver's refresh, then ``b0``, ``A`` and its
        preconditioner again.  ``u, v, a`` and ``t`` are kept."""
        s = self.solver
        s.refresh()
        with torch.no_grad():
            self._mass.refresh()
            s._gradient(s._zero, self._b0)
            self._b0.neg_()
        self._bind_step()
        self._key = s._state_key()

    def _ensure(self):
        if self._key is None or self._key != self.solver._state_key():
            self.refresh()

    def _apply_k(self, p, q):
        check(_lib.lib().hfem_cg_apply(self.solver._h, ptr(p), ptr(q), ptr(self._pq), stream_ptr(self.device)), "hfem_cg_apply")

    def _apply_a(self, p, q):
        check(_lib.lib().hfem_cg_apply(self._h, ptr(p), ptr(q), ptr(self._pq), stream_ptr(self.device)), "hfem_cg_apply")

    def _apply_m(self, p, q):
        self._mass.apply(p, q)

    def operator_apply(self, p: torch.Tensor, coefficients=None):
        """Standalone ``q = A p`` over the free u rows and ``p^T A p`` (0-d device tensor); ``p`` is fp64 ``[n_u, 2]`` in
        storage order.  ``coefficients = (c_K, c_M)``: the operator ``c_K K + c_M rho M`` instead of the step's (the handle is
        bound to the step's again afterwards).  For tests and measurements."""
        self._ensure()
        p = _lib.require_gpu_tensor(p.detach(), "p", F64)
        q = torch.empty_like(p)
        pq = torch.empty((), dtype=F64, device=self.device)
        if coefficients is not None:
            self._bind(float(coefficients[0]), float(coefficients[1]))
        try:
            check(_lib.lib().hfem_cg_apply(self._h, ptr(p), ptr(q), ptr(pq), stream_ptr(self.device)), "hfem_cg_apply")
        finally:
            if coefficients is not None:
                self._bind(self.c_k, self.c_m)
        return q, pq

    def operator_blocks(self, coefficients=None) -> torch.Tensor:
        """The 2x2 diagonal blocks ``{A_xx, A_xy, A_yy}`` ``[n_u, 3]`` of ``hfem_cg_setup_shifted`` (``coefficients`` as
        ``operator_apply``).  For tests and measurements."""
        self._ensure()
        if coefficients is None:
            return self.diag.clone()
        self._bind(float(coefficients[0]), float(coefficients[1]))
        out = self.diag.clone()
        self._bind(self.c_k, self.c_m)
        return out

    def precondition(self, r: torch.Tensor):
        """``z = V(r)``: one V-cycle of the hierarchy on ``A`` (``precond="amg"`` only).  For tests and measurements."""
        if self._amg is None:
            raise ValueError("precondition(): precond='amg' only")
        self._ensure()
        r = _lib.require_gpu_tensor(r.detach().contiguous(), "r", F64)
        z = torch.empty_like(r)
        check(_lib.lib().hfem_amg_vcycle(self._amg._h, ptr(r), ptr(z), stream_ptr(self.device)), "hfem_amg_vcycle")
        return z

    def assemble_operator(self, coefficients=None) -> torch.Tensor:
        """``A`` at the current coordinates: fp64 ``torch.sparse_bsr_tensor`` with 2x2 blocks over the free u rows in storage
        order, as ``solve.assemble_stiffness`` gives ``K`` (one thread per row, no atomics: bit-deterministic).
        ``coefficients`` as ``operator_apply``."""
        self._ensure()
        c_k, c_m = (self.c_k, self.c_m) if coefficients is None else (float(coefficients[0]), float(coefficients[1]))
        host = amg_host(self.model)
        a = _AmgDevice(host, self.device, self.phys)
        s = self.solver
        mat, W = self._mat()
        a.assemble_shifted(s._xf, s._xfix, mat, W, c_k, c_m * self.density, self.lumped)
        vals = a.values(0, 0).view(-1, 2, 2).clone()
        n = host.levels[0][0]
        i64 = dict(dtype=torch.int64, device=self.device)
        crow = torch.as_tensor(host.array(0, 0), **i64)
        col = torch.as_tensor(host.array(0, 1), **i64)
        return torch.sparse_bsr_tensor(crow, col, vals, size=(2 * n, 2 * n))

    # ---- one linear solve A a = rhs on the bound coefficients, warm-started from self.a
    def _read_status(self):
        check(_lib.lib().hfem_cg_status(self._h, self._status, stream_ptr(self.device)), "hfem_cg_status")
        return list(self._status)

    def _iterate(self, amg):
        args = (ptr(self.a), self.iters_per_graph, stream_ptr(self.device))
        if amg is None:
            check(_lib.lib().hfem_cg_iterate(self._h, *args), "hfem_cg_iterate")
        else:
            check(_lib.lib().hfem_cg_iterate_amg(self._h, amg._h, *args), "hfem_cg_iterate_amg")

    def _replay(self, amg):
        # a captured launch holds the operator's coefficients by value: one graph per (c_K, c_M, preconditioner)
        key = (self._bound, amg is not None)
        if key not in self._graphs:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                        # captured, not executed
                self._iterate(amg)
            self._graphs[key] = g
        self._graphs[key].replay()

    def _solve(self, load, alpha_r, amg, t):
        """rhs = load b0 - K w - alpha_r M v~ from ``self._w`` / ``self._vt``; ``self.a`` <- the solution of A a = rhs."""
        lib, d, s = _lib.lib(), _lib.dev_index(self.device), stream_ptr(self.device)
        self._apply_k(self._w, self._kw)
        if alpha_r != 0.0:
            self._apply_m(self._vt, self._mv)
        direct = self.lumped and self._bound[0] == 0.0
        if direct:
            self._aa.zero_()
        else:
            self._apply_a(self.a, self._aa)
        check(lib.hfem_newmark_rhs(d, ptr(self._b0), ptr(self._kw), ptr(self._mv) if alpha_r != 0.0 else None, ptr(self._aa),
                                   self.len, float(load), alpha_r, ptr(self._g0), ptr(self._gz), s), "hfem_newmark_rhs")
        if direct:                                           # A is block diagonal: a = D^-1 rhs, no CG
            check(lib.hfem_block_jacobi_apply(d, ptr(self.diag), ptr(self._gz), 1, self.len, ptr(self.a), s),
                  "hfem_block_jacobi_apply")
            return StepInfo(t=t, iterations=0, residual_norm=0.0, rhs_norm=float(torch.linalg.vector_norm(self._gz)),
                            converged=True, reason="direct")
        args = (ptr(self._g0), ptr(self._gz), self.rtol, self.atol, self.max_iter, s)
        if amg is None:
            check(lib.hfem_cg_start(self._h, *args), "hfem_cg_start")
        else:
            check(lib.hfem_cg_start_amg(self._h, amg._h, *args), "hfem_cg_start_amg")
        st = self._read_status()
        while not st[ST_HALTED] and st[ST_ITER] < self.max_iter:
            self._replay(amg)
            st = self._read_status()
        reason = _REASONS.get(int(st[ST_REASON]), "max_iter")
        return StepInfo(t=t, iterations=int(st[ST_ITER]), residual_norm=float(st[ST_RNORM]), rhs_norm=float(st[ST_FNORM]),
                        converged=reason in ("rtol", "atol"), reason=reason)

    # ---- time stepping
    def set_state(self, u: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None) -> StepInfo:
        """Initial displacement and velocity (default ``model.u_free`` and 0), ``t = 0``, and the initial acceleration from
        ``M a0 = load(0) b0 - K u0 - C v0``.  Returns that solve's ``StepInfo``."""
        self._ensure()
        lib, d, s = _lib.lib(), _lib.dev_index(self.device), stream_ptr(self.device)
        with torch.no_grad():
            self.u.copy_(self.model.u_free.detach() if u is None else self._row_tensor(u, "u"))
            if v is None:
                self.v.zero_()
            else:
                self.v.copy_(self._row_tensor(v, "v"))
            self.a.zero_()
            self.t = 0.0
            # dt = 0 in the predictor: u~ = u, v~ = v, w = u + beta_R v
            check(lib.hfem_newmark_predict(d, ptr(self.u), ptr(self.v), ptr(self.a), self.len, 0.0, self.beta, self.gamma,
                                           self.beta_r, ptr(self._ut), ptr(self._vt), ptr(self._w), s), "hfem_newmark_predict")
            self._bind(0.0, 1.0)                             # A = M: block Jacobi at the most, never a hierarchy
            info = self._solve(self.load(0.0), self.alpha_r, None, 0.0)
            self._bind(self.c_k, self.c_m)                   # the hierarchy of the last refresh is still the one of A
        self._started = True
        return info

    def _row_tensor(self, x, name):
        x = x.detach()
        if tuple(x.shape) != (self.n_u, 2):
            raise ValueError(f"{name}: a tensor [{self.n_u}, 2] in the storage order of u_free")
        return x.to(device=self.device, dtype=F64)

    def step(self, n: int = 1):
        """Advance ``n`` steps; returns their ``StepInfo`` in order.  ``model.u_free`` receives ``u`` at the end."""
        if int(n) < 0:
            raise ValueError("n must be >= 0")
        if not self._started:
            self.set_state()
        self._ensure()
        lib, d, s = _lib.lib(), _lib.dev_index(self.device), stream_ptr(self.device)
        out = []
        with torch.no_grad():
            for _ in range(int(n)):
                check(lib.hfem_newmark_predict(d, ptr(self.u), ptr(self.v), ptr(self.a), self.len, self.dt, self.beta,
                                               self.gamma, self.beta_r, ptr(self._ut), ptr(self._vt), ptr(self._w), s),
                      "hfem_newmark_predict")
                t1 = self.t + self.dt
                info = self._solve(self.load(t1), self.alpha_r, self._amg, t1)
                check(lib.hfem_newmark_correct(d, ptr(self._ut), ptr(self._vt), ptr(self.a), self.len, self.dt, self.beta,
                                               self.gamma, ptr(self.u), ptr(self.v), s), "hfem_newmark_correct")
                self.t = t1
                out.append(info)
            self.model.u_free.copy_(self.u)                  # rounds once for fp32 models
        return out

    def energy(self) -> dict:
        """``kinetic`` = 1/2 v^T M v, ``strain`` = 1/2 u^T K u, ``work`` = load(t) u^T b0 and ``total`` = kinetic + strain -
        work at the current state (Python floats).  Runs on demand: one mass and one stiffness apply, the dots by
        ``hfem_block_gram``."""
        self._ensure()
        S = self._stack
        with torch.no_grad():
            S[0].copy_(self.v); S[1].copy_(self.u); S[2].copy_(self.u); S[5].copy_(self._b0)
            self._apply_m(S[0], S[3])
            self._apply_k(S[1], S[4])
            check(_lib.lib().hfem_block_gram(_lib.dev_index(self.device), ptr(S[0]), 3, ptr(S[3]), 3, self.len,
                                             ptr(self._gram_partials), ptr(self._gram), stream_ptr(self.device)), "hfem_block_gram")
            g = self._gram.cpu().numpy().reshape(3, 3)
        kin, strain, work = 0.5 * float(g[0, 0]), 0.5 * float(g[1, 1]), float(self.load(self.t)) * float(g[2, 2])
        return dict(kinetic=kin, strain=strain, work=work, total=kin + strain - work)


def transient_(model, loss_fn, n_steps: int, dt: float, callback: Optional[Callable] = None, **kw):
    """One-shot ``NewmarkSolver(model, loss_fn, dt, **kw)``: ``set_state()`` from ``model.u_free`` at rest, then ``n_steps``
    steps, ``callback(solver)`` after every one.  Returns ``(solver, [StepInfo])``."""
    s = NewmarkSolver(model, loss_fn, dt, **kw)
    s.set_state()
    infos = []
    for _ in range(int(n_steps)):
        infos += s.step(1)
        if callback is not None:
            callback(s)
    return s, infos


# ---------------------------------------------------------------- finite strain
@dataclass
class HyperStepInfo(StepInfo):
    """``StepInfo`` of a finite-strain step.  ``iterations``: CG iterations summed over the step's Newton iterations;
    ``residual_norm``: ``||R||_2`` at the returned acceleration, ``rhs_norm``: ``||R(a = 0)||_2``; ``reason``: ``"rtol"`` /
    ``"atol"``, ``"max_newton"``, ``"line_search"``, ``"inverted"`` or ``"direct"``.  ``min_J``: the smallest det F of the state
    the step arrived at; ``history``: one dict per Newton iteration, ``NewtonInfo.history``'s keys (``energy`` is the incremental
    potential ``Phi``, ``grad_norm`` is ``||R||``)."""
    newton_iterations: int = 0
    min_J: float = float("nan")
    history: List[dict] = field(default_factory=list)


class HyperNewmarkSolver:
    """Newmark time stepping at finite strain (total Lagrangian) for a TRI3 model under a ``NeoHookeanLoss2D`` or a
    QUAD4 model under a ``Quad4NeoHookeanLoss2D``; an ``EnergyLoss2D`` belongs to ``NewmarkSolver``.

    ``M u'' + alpha_R M u' + f_int(u) = load(t) b_ext`` over the free ``u`` rows at the model's current coordinates (the reference
    configuration): ``f_int`` is the gradient of the Neo-Hookean energy launch with no forces, ``b_ext = f_int(0) - g(0)`` the dead
    loads alone (the ``u_fixed`` term is in both launches at ``u_free = 0`` and cancels; formed once per refresh), ``M`` the mass of
    ``hfem_mass_apply``.  Damping is mass-proportional: ``rayleigh = (alpha_R, 0)``; ``beta_R != 0`` raises ``ValueError``.  Per
    step, with ``c_K = beta dt^2`` and ``c_M = 1 + gamma dt alpha_R``::

        u~ = u + dt v + dt^2 (1/2 - beta) a      v~ = v + dt (1 - gamma) a
        R(a+) = c_M M a+ + alpha_R M v~ + f_int(u~ + c_K a+) - load(t + dt) b_ext = 0
        u+ = u~ + beta dt^2 a+                   v+ = v~ + gamma dt a+

    Newton starts from the previous ``a`` (from ``u+ = u`` where that start has an inverted element) and stops at
    ``||R|| <= max(rtol ||R(a = 0)||, atol)`` (tested first in every
    iteration) or after ``max_newton`` iterations.  Every iteration solves ``A d = -R`` with ``A = c_M M + c_K K_T(u~ + c_K a)``
    by the PCG driver with ``newton.py``'s Eisenstat-Walker forcing (``eta_max``), truncation rules and ``cg_max_iter``, then
    backtracks on the incremental potential ``Phi(a) = Pi_int(u(a)) - load b_ext . u(a) + c_K [1/2 c_M a^T M a + alpha_R a^T M v~]``
    (``grad Phi = c_K R``) with ``newton.py``'s Armijo test (``armijo``, ``max_backtracks``; ``+inf`` from an inverted trial is an
    ordinary rejection).
    Its rounding slack ``4 eps |Phi|`` is taken over the magnitudes of Phi's terms, ``|Pi_int| + |load b_ext . u| + c_K (...)``:
    strain energy and work cancel to a Phi some eighty times smaller than either, and the slack has to cover the rounding of
    what is summed, not of the sum -- with ``|Phi|`` itself the test rejects every step once ``||R||`` is within 1e-9 of
    ``||R(a = 0)||``; where nothing cancels the two are the same.
    ``M d`` is formed once per Newton iteration, so a trial costs one energy
    launch, one vector pass and one ``hfem_block_gram``.  ``precond``: ``"block_jacobi"`` (the 2x2 blocks of ``A``, rebuilt at
    every linearisation), ``"none"``, or ``"amg"`` (the hierarchy of ``c_K K_lin + c_M M`` with the small-strain material, set up
    once per refresh: a fixed SPD preconditioner for the varying ``A``; needs Dirichlet rows and ``c_K > 0``).  With a lumped mass
    and ``c_K = 0`` -- the initial acceleration, and every step of explicit central difference (``beta = 0``) -- ``A`` is block
    diagonal: one energy launch and one ``hfem_block_jacobi_apply`` (``reason == "direct"``, no iterations).

    ``rtol`` defaults to ``newton.py``'s 1e-8, not to ``NewmarkSolver``'s 1e-10: ``f_int`` is a sum of element forces that cancel,
    and on the 10^6-element meshes one step in three at ``dt = T1/400`` cannot bring ``||R||`` below 1e-10 ``||R(a = 0)||`` at all
    and runs into ``max_newton``.  A step that ends ``"max_newton"`` is taken, as ``NewmarkSolver`` takes an
    unconverged CG solve.

    A step that ends with ``reason`` ``"inverted"`` (both starts have an element with det F <= 0) or
    ``"line_search"`` (no trial was accepted) leaves ``u, v, a, t`` untouched and ``step()`` returns there.

    The surface is ``NewmarkSolver``'s: ``set_state(u, v)``, ``step(n)``, ``.t/.u/.v/.a``, ``refresh()``, ``energy()``,
    ``operator_apply``, ``operator_blocks``; ``model.u_free`` receives ``u`` at the end of every ``step()`` call (fp32 models are
    stepped in fp64 and rounded once there).  It owns a ``NewtonKrylovSolver`` / ``Quad4NewtonKrylovSolver`` for the plan, the
    force tables, the energy launch, the PCG handle and the refresh key.  Not bitwise reproducible (LDS atomics)."""

    def __init__(self, model, loss_fn, dt: float, density: float = 1.0, mass: str = "consistent", beta: float = 0.25,
                 gamma: float = 0.5, rayleigh=(0.0, 0.0), load: Optional[Callable] = None, precond: str = "block_jacobi",
                 rtol: float = 1e-8, atol: float = 0.0, max_newton: int = 50, cg_max_iter: Optional[int] = None,
                 iters_per_graph: int = 16, eta_max: float = 0.1, armijo: float = 1e-4, max_backtracks: int = 30,
                 b_force: Optional[Callable] = None, t_force: Optional[Callable] = None):
        from .newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver
        npe = getattr(model, "nodes_per_element", 3)
        quad = isinstance(loss_fn, Quad4NeoHookeanLoss2D)
        if not isinstance(loss_fn, NeoHookeanLoss2D):
            raise NotImplementedError("HyperNewmarkSolver: NeoHookeanLoss2D / Quad4NeoHookeanLoss2D only (an EnergyLoss2D is "
                                      "linear: NewmarkSolver / transient_ step it)")
        if not hasattr(model, "_conn32") or (npe, quad) not in ((3, False), (4, True)):
            raise NotImplementedError("HyperNewmarkSolver: a TRI3 model under a NeoHookeanLoss2D or a QUAD4 model under a "
                                      "Quad4NeoHookeanLoss2D")
        dt, beta, gamma, density, alpha_r, beta_r = _check_newmark(dt, beta, gamma, density, mass, precond, iters_per_graph, rtol,
                                                                   atol, rayleigh)
        if beta_r != 0.0:
            raise ValueError("HyperNewmarkSolver: damping is mass-proportional only, rayleigh = (alpha_R, 0) (a stiffness-"
                             "proportional term would need a choice of K)")
        if not 0.0 < eta_max < 1.0:
            raise ValueError("eta_max must be in (0, 1)")
        c_k, c_m = beta * dt * dt, 1.0 + gamma * dt * alpha_r
        if precond == "amg" and int(model._idx_udir.shape[0]) == 0:
            raise ValueError("precond='amg' needs Dirichlet rows (rigid-body modes are out of scope)")
        if precond == "amg" and c_k == 0.0:
            raise ValueError("precond='amg' with c_K = beta dt^2 = 0: A is a pure mass matrix and needs no hierarchy (use "
                             "'block_jacobi')")
        cls = Quad4NewtonKrylovSolver if quad else NewtonKrylovSolver
        # refuses a CPU model: there is no CPU fallback.  Its own preconditioner is never "amg": the hierarchy here is the
        # shifted one, owned below and lent to it for the inner solves of a step
        self.newton = nw = cls(model, loss_fn, b_force=b_force, t_force=t_force,
                               precond="none" if precond == "none" else "block_jacobi", max_newton=max_newton,
                               cg_max_iter=cg_max_iter, iters_per_graph=iters_per_graph, eta_max=eta_max, armijo=armijo,
                               max_backtracks=max_backtracks)
        self.model, self.loss_fn, self.npe = model, loss_fn, npe
        self.dt, self.density, self.mass, self.beta, self.gamma = dt, density, mass, beta, gamma
        self.alpha_r, self.beta_r, self.c_k, self.c_m = alpha_r, 0.0, c_k, c_m
        self.load = (lambda t: 1.0) if load is None else load
        self.precond, self.rtol, self.atol = precond, float(rtol), float(atol)
        self.max_newton, self.iters_per_graph = int(max_newton), int(iters_per_graph)
        self.armijo, self.max_backtracks, self.eta_max = float(armijo), int(max_backtracks), float(eta_max)
        self.lumped = mass == "lumped"
        self.device = dev = nw.device
        self.n_u = n_u = nw.n_u
        self.len = 2 * n_u
        self._amg = _AmgDevice(amg_host(model), dev, True) if precond == "amg" else None
        self._mass = _MassOperator(model, npe, dev, n_u, density, self.lumped)
        z = dict(dtype=F64, device=dev)
        new = lambda: torch.zeros((n_u, 2), **z)
        self.u, self.v, self.a = new(), new(), new()
        self._ut, self._vt, self._w, self._an, self._ma, self._md, self._f = new(), new(), new(), new(), new(), new(), new()
        self._ta = torch.zeros((2, n_u, 2), **z)          # trial rows {u_t, a_t}
        self._tb = torch.zeros((3, n_u, 2), **z)          # {b_ext, (M a)_t, M v~}: Phi's dots are the Gram of the two stacks
        self._b = self._tb[0]
        self._stack = torch.zeros((4, n_u, 2), **z)       # energy(): [v, u | M v, b_ext]
        self._gram = torch.zeros(9, **z)
        self._gram_partials = torch.empty(GRAM_PARTIALS, **z)
        self.diag = nw.diag                               # the 2x2 blocks {A_xx, A_xy, A_yy} of the last linearisation
        self._graphs = {}
        self._bound = None                                # (c_k, c_m) of a block-diagonal binding the direct path may reuse
        self._int = None                                  # the force tables of the internal-energy launch
        self._key = None
        self._started = False
        self.t = 0.0

    # ---- refresh
    def refresh(self):
        """Coordinates, ``u_fixed`` or the forces changed: the Newton solver's refresh, then ``b_ext``, the mass coordinates and
        the hierarchy again.  ``u, v, a`` and ``t`` are kept."""
        nw = self.newton
        nw.refresh()                                         # nw._gz = g(u_free = 0) of the full launch
        with torch.no_grad():
            self._int = nw._internal_tables()
            self._mass.refresh()
            nw._energy(nw._zero, self._f, self._int)
            torch.sub(self._f, nw._gz, out=self._b)          # dead loads are linear in u: exact up to rounding
            if self._amg is not None:
                lam, mu = self.loss_fn.lame
                self._amg.setup_shifted(nw._xf, nw._xfix, (C.c_double * 4)(lam + 2 * mu, lam, lam + 2 * mu, mu),
                                        float(self.loss_fn._W), self.c_k, self.c_m * self.density, self.lumped)
        self._bound = None
        self._key = nw._state_key()

    def _ensure(self):
        if self._key is None or self._key != self.newton._state_key():
            self.refresh()

    # ---- launches
    def _linearise(self, c_k, c_m, u, jacobi=True):
        """Bind the PCG handle to ``c_k K_T(u) + c_m rho M`` (``u``: a solver-owned buffer) and build its blocks there."""
        nw = self.newton
        check(_lib.lib().hfem_cg_setup_hyper_shifted(
            nw._h, ptr(nw._xf), ptr(nw._xfix) if nw._xfix.numel() else None, ptr(u), ptr(nw._ufix) if nw._ufix.numel() else None,
            nw._lame, float(self.loss_fn._W), c_k, c_m * self.density, 1 if self.lumped else 0, 1 if jacobi else 0, ptr(self.diag),
            ptr(nw._info), stream_ptr(self.device)), "hfem_cg_setup_hyper_shifted")
        self._bound = (c_k, c_m)

    def _f_int(self, u, g):
        """``g = f_int(u)``; -> (Pi_int, min J, inverted count)"""
        self.newton._energy(u, g, self._int)
        return self.newton._out.tolist()

    def _dots(self, a, ma, b, mb):
        check(_lib.lib().hfem_block_gram(_lib.dev_index(self.device), ptr(a), ma, ptr(b), mb, self.len, ptr(self._gram_partials),
                                         ptr(self._gram), stream_ptr(self.device)), "hfem_block_gram")
        return self._gram[:ma * mb].cpu().numpy().reshape(ma, mb)

    def _dot(self, x, y):
        return float(self._dots(x, 1, y, 1)[0, 0])

    def _residual(self, ma, f, c_m, alpha_r, load, r, neg_r=None):
        check(_lib.lib().hfem_newmark_residual(_lib.dev_index(self.device), ptr(ma), ptr(self._tb[2]) if alpha_r != 0.0 else None,
                                               ptr(f), ptr(self._b), self.len, c_m, alpha_r, float(load), ptr(r), ptr(neg_r),
                                               stream_ptr(self.device)), "hfem_newmark_residual")

    def _trial(self, s, c_k):
        check(_lib.lib().hfem_newmark_trial(_lib.dev_index(self.device), ptr(self._an), ptr(self.newton._delta), ptr(self._ut),
                                            ptr(self._ma), ptr(self._md), self.len, s, c_k, ptr(self._ta[1]), ptr(self._ta[0]),
                                            ptr(self._tb[1]), stream_ptr(self.device)), "hfem_newmark_trial")

    def _phi(self, pi, load, c_k, c_m, alpha_r):
        """The incremental potential of the trial rows from their energy ``pi`` and one Gram of the two stacks.
        -> (Phi, the sum of the magnitudes of its terms: the scale its rounding error has)"""
        g = self._dots(self._ta, 2, self._tb, 3)
        work, inertia, damping = load * float(g[0, 0]), c_k * 0.5 * c_m * float(g[1, 1]), c_k * alpha_r * float(g[1, 2])
        return pi - work + inertia + damping, abs(pi) + abs(work) + abs(inertia) + abs(damping)

    def _inner(self, eta, amg, key):
        """The Newton solver's truncated PCG on the bound operator, ``R`` in its ``_g``, the direction in its ``_delta``; one
        captured graph per (c_K, c_M, preconditioner)."""
        nw = self.newton
        nw._amg, nw._graph = amg, self._graphs.get(key)
        try:
            return nw._inner(eta)
        finally:
            self._graphs[key] = nw._graph
            nw._amg, nw._graph = None, None

    # ---- one solve for a+ from self._ut / self._vt, warm-started from self.a, into self._an
    def _solve(self, load, c_k, c_m, alpha_r, amg, t):
        from .newton import EPS
        nw, load = self.newton, float(load)
        info = lambda **kw: HyperStepInfo(t=t, **kw)
        if alpha_r != 0.0:
            self._mass.apply(self._vt, self._tb[2])
        # R(a = 0): the norm of the stopping test (one energy launch)
        pi0, mj0, inv0 = self._f_int(self._ut, self._f)
        self._residual(nw._zero, self._f, c_m, alpha_r, load, nw._g, nw._gt)
        rhs_norm = math.sqrt(self._dot(nw._g, nw._g))
        if self.lumped and c_k == 0.0:                       # A is block diagonal and u(a) = u~: a = D^-1 (-R(0)), no Newton
            if inv0 > 0:
                return info(iterations=0, residual_norm=rhs_norm, rhs_norm=rhs_norm, converged=False, reason="inverted", min_J=mj0)
            if self._bound != (0.0, c_m):
                self._linearise(0.0, c_m, self._ut)
            check(_lib.lib().hfem_block_jacobi_apply(_lib.dev_index(self.device), ptr(self.diag), ptr(nw._gt), 1, self.len,
                                                     ptr(self._an), stream_ptr(self.device)), "hfem_block_jacobi_apply")
            return info(iterations=0, residual_norm=0.0, rhs_norm=rhs_norm, converged=True, reason="direct", min_J=mj0)
        tol = max(self.rtol * rhs_norm, self.atol)
        hist: List[dict] = []
        # the start: a = the previous acceleration
        self._an.copy_(self.a)
        self._mass.apply(self._an, self._ma)
        nw._delta.zero_(); self._md.zero_()
        self._trial(0.0, c_k)
        pi, min_j, inv = self._f_int(self._ta[0], self._f)
        if inv > 0 and c_k > 0.0:
            # u~ + c_K a extrapolates with the previous acceleration, which can overshoot into an inverted state although the
            # step has a solution: start at u+ = u, the state the step comes from, a = (u - u~) / c_K
            torch.sub(self.u, self._ut, out=self._an)
            self._an.mul_(1.0 / c_k)
            self._mass.apply(self._an, self._ma)
            self._trial(0.0, c_k)
            pi, min_j, inv = self._f_int(self._ta[0], self._f)
        if inv > 0:
            return info(iterations=0, residual_norm=float("inf"), rhs_norm=rhs_norm, converged=False, reason="inverted", min_J=min_j)
        phi, mag = self._phi(pi, load, c_k, c_m, alpha_r)
        nw._u.copy_(self._ta[0])
        self._residual(self._ma, self._f, c_m, alpha_r, load, nw._g)
        gn = math.sqrt(self._dot(nw._g, nw._g))
        k, cg_total, gn_prev, reason = 0, 0, None, ""
        key = (c_k, c_m, amg is not None, self.precond)
        while True:
            if gn <= tol:
                reason = "rtol" if self.rtol * rhs_norm >= self.atol else "atol"
                break
            if k >= self.max_newton:
                reason = "max_newton"
                break
            self._linearise(c_k, c_m, nw._u, jacobi=self.precond != "none" and amg is None)
            eta = self.eta_max if gn_prev is None else min(max(0.9 * (gn / gn_prev) ** 2, 1e-12), self.eta_max)
            its, halt = self._inner(eta, amg, key)
            cg_total += its
            self._mass.apply(nw._delta, self._md)
            slope = c_k * self._dot(nw._g, nw._delta)
            s, accepted = 1.0, False
            for _ in range(self.max_backtracks + 1):
                self._trial(s, c_k)
                pi_t, mj_t, _ = self._f_int(self._ta[0], self._f)
                phi_t, mag_t = self._phi(pi_t, load, c_k, c_m, alpha_r) if math.isfinite(pi_t) else (float("inf"), mag)
                if math.isfinite(phi_t) and phi_t <= phi + self.armijo * s * slope + 4.0 * EPS * mag:
                    accepted = True
                    break
                s *= 0.5
            hist.append(dict(energy=phi, grad_norm=gn, eta=eta, cg_iterations=its, cg_reason=halt, step=s if accepted else 0.0,
                             min_J=mj_t if accepted else min_j))
            if not accepted:
                reason = "line_search"
                break
            self._an.copy_(self._ta[1]); nw._u.copy_(self._ta[0]); self._ma.copy_(self._tb[1])
            self._residual(self._ma, self._f, c_m, alpha_r, load, nw._g)
            gn_prev, phi, mag, min_j = gn, phi_t, mag_t, mj_t
            gn = math.sqrt(self._dot(nw._g, nw._g))
            k += 1
        return info(iterations=cg_total, residual_norm=gn, rhs_norm=rhs_norm, converged=reason in ("rtol", "atol"), reason=reason,
                    newton_iterations=k, min_J=min_j, history=hist)

    # ---- time stepping
    def _row_tensor(self, x, name):
        x = x.detach()
        if tuple(x.shape) != (self.n_u, 2):
            raise ValueError(f"{name}: a tensor [{self.n_u}, 2] in the storage order of u_free")
        return x.to(device=self.device, dtype=F64)

    def _predict(self, dt):
        check(_lib.lib().hfem_newmark_predict(_lib.dev_index(self.device), ptr(self.u), ptr(self.v), ptr(self.a), self.len, dt,
                                              self.beta, self.gamma, 0.0, ptr(self._ut), ptr(self._vt), ptr(self._w),
                                              stream_ptr(self.device)), "hfem_newmark_predict")

    def set_state(self, u: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None) -> HyperStepInfo:
        """Initial displacement and velocity (default ``model.u_free`` and 0), ``t = 0``, and the initial acceleration from
        ``M a0 = load(0) b_ext - f_int(u0) - alpha_R M v0`` (the same handle bound with ``c_K = 0``: block Jacobi at the most).
        Returns that solve's ``HyperStepInfo``."""
        self._ensure()
        with torch.no_grad():
            self.u.copy_(self.model.u_free.detach() if u is None else self._row_tensor(u, "u"))
            if v is None:
                self.v.zero_()
            else:
                self.v.copy_(self._row_tensor(v, "v"))
            self.a.zero_()
            self.t = 0.0
            self._predict(0.0)                               # u~ = u, v~ = v
            info = self._solve(self.load(0.0), 0.0, 1.0, self.alpha_r, None, 0.0)
            if info.reason != "inverted":
                self.a.copy_(self._an)
        self._started = True
        return info

    def step(self, n: int = 1):
        """Advance ``n`` steps; returns their ``HyperStepInfo`` in order and stops behind a step that ended ``"inverted"`` or
        ``"line_search"`` (the state is the one before it).  ``model.u_free`` receives ``u`` at the end, also when a later step of the
        call stopped it; a call whose first step fails writes nothing."""
        if int(n) < 0:
            raise ValueError("n must be >= 0")
        if not self._started:
            self.set_state()
        self._ensure()
        out, advanced = [], int(n) == 0
        with torch.no_grad():
            for _ in range(int(n)):
                self._predict(self.dt)
                t1 = self.t + self.dt
                info = self._solve(self.load(t1), self.c_k, self.c_m, self.alpha_r, self._amg, t1)
                out.append(info)
                if info.reason in ("inverted", "line_search"):
                    info.t = self.t
                    break                                    # u, v, a, t as they were before this step
                self.a.copy_(self._an)
                check(_lib.lib().hfem_newmark_correct(_lib.dev_index(self.device), ptr(self._ut), ptr(self._vt), ptr(self.a),
                                                      self.len, self.dt, self.beta, self.gamma, ptr(self.u), ptr(self.v),
                                                      stream_ptr(self.device)), "hfem_newmark_correct")
                self.t = t1
                advanced = True
            if advanced:                                     # a call whose first step fails leaves model.u_free bit-unchanged
                self.model.u_free.copy_(self.u)              # rounds once for fp32 models
        return out

    def energy(self) -> dict:
        """``kinetic`` = 1/2 v^T M v, ``strain`` = Pi_int(u), ``work`` = load(t) b_ext . u and ``total`` = kinetic + strain - work
        at the current state (Python floats).  On demand: one mass apply, one energy launch, the dots by ``hfem_block_gram``."""
        self._ensure()
        S = self._stack
        with torch.no_grad():
            S[0].copy_(self.v); S[1].copy_(self.u); S[3].copy_(self._b)
            self._mass.apply(S[0], S[2])
            strain = self._f_int(S[1], self._f)[0]
            g = self._dots(S[0], 2, S[2], 2)
        kin, work = 0.5 * float(g[0, 0]), float(self.load(self.t)) * float(g[1, 1])
        return dict(kinetic=kin, strain=strain, work=work, total=kin + strain - work)

    # ---- test and measurement helpers
    def _bind_at(self, coefficients, u):
        self._ensure()
        c_k, c_m = (self.c_k, self.c_m) if coefficients is None else (float(coefficients[0]), float(coefficients[1]))
        nw = self.newton
        with torch.no_grad():
            nw._u.copy_(self.u if u is None else self._row_tensor(u, "u"))
        self._linearise(c_k, c_m, nw._u)
        self._bound = None

    def operator_apply(self, p: torch.Tensor, coefficients=None, u: Optional[torch.Tensor] = None):
        """Standalone ``q = A p`` and ``p^T A p`` (0-d device tensor) with ``A = c_K K_T(u) + c_M rho M``: ``p`` fp64 ``[n_u, 2]``
        in storage order, ``coefficients = (c_K, c_M)`` (default: the step's), ``u``: the linearisation point (default: the
        current ``.u``).  Re-linearises (``diag`` and ``info`` follow).  For tests and measurements."""
        self._bind_at(coefficients, u)
        p = _lib.require_gpu_tensor(p.detach(), "p", F64)
        q = torch.empty_like(p)
        pq = torch.empty((), dtype=F64, device=self.device)
        check(_lib.lib().hfem_cg_apply(self.newton._h, ptr(p), ptr(q), ptr(pq), stream_ptr(self.device)), "hfem_cg_apply")
        return q, pq

    def operator_blocks(self, coefficients=None, u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 2x2 diagonal blocks ``{A_xx, A_xy, A_yy}`` ``[n_u, 3]`` of ``hfem_cg_setup_hyper_shifted`` (arguments as
        ``operator_apply``).  For tests and measurements."""
        self._bind_at(coefficients, u)
        return self.diag.clone()

    @property
    def info(self) -> torch.Tensor:
        """``{min J, number of elements with J <= 0}`` of the last linearisation (fp64 device tensor)."""
        return self.newton._info


def hyper_transient_(model, loss_fn, n_steps: int, dt: float, callback: Optional[Callable] = None, **kw):
    """One-shot ``HyperNewmarkSolver(model, loss_fn, dt, **kw)``: ``set_state()`` from ``model.u_free`` at rest, then ``n_steps``
    steps, ``callback(solver)`` after every one; stops behind a step that ended ``"inverted"`` or ``"line_search"``.  Returns ``(solver, [HyperStepInfo])``."""
    s = HyperNewmarkSolver(model, loss_fn, dt, **kw)
    s.set_state()
    infos = []
    for _ in range(int(n_steps)):
        infos += s.step(1)
        if infos[-1].reason in ("inverted", "line_search"):  # the state did not move: another step would be the same one
            break
        if callback is not None:
            callback(s)
    return s, infos
