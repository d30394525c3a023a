"""Harmonic frequency response of a TRI3 or QUAD4 model: the steady state under a load ``Re(b e^{i omega t})`` with damping.

Over the free ``u`` rows, with ``K`` the operator the frozen-mesh solver applies at the model's CURRENT coordinates
(``hfem_cg_apply``), ``M`` the consistent or lumped mass of ``hfem_mass_apply`` (density rho), Rayleigh damping
``C = alpha_R M + beta_R K`` and structural damping ``i eta K``::

    (K + i omega C - omega^2 M) u^ = b^      i.e.      A u^ = b^,   A = z_K K + z_M M,
    z_K = 1 + i (omega beta_R + eta),        z_M = rho (-omega^2 + i omega alpha_R)

``A`` is complex symmetric, not Hermitian, and its real part is indefinite above the first resonance: the shifted operator and
the PCG driver of ``NewmarkSolver`` do not apply.  ``csrc/harmonic.hip`` holds the two new pieces: the complex apply (sibling
kernels of the ``MASS`` instances of ``csrc/tri3_cg.hip`` / ``csrc/quad4_cg.hip`` on the same tile plans: one gather per tile,
both planes of ``p`` in LDS, ``K_e p_r, K_e p_i, M_e p_r, M_e p_i`` formed in the slot loop and combined with the four run-time
coefficients) and a preconditioned COCG driver (conjugate orthogonal conjugate gradients: CG in the unconjugated bilinear form)
whose scalars are reduced and consumed on the device.  The preconditioner is REAL and SPD, ``T ~ (K + omega_p^2 rho M)^-1`` -- the
sign-flipped shift -- applied to the real and the imaginary plane alike: one V-cycle of a smoothed-aggregation hierarchy on it
(``hfem_amg_setup_shifted``), its 2x2 diagonal blocks (``hfem_cg_setup_shifted``'s ``diag_out``), or nothing.

On the device a complex vector is an fp64 block vector ``[2][n_u][2]`` (plane 0 real, plane 1 imaginary); this module takes and
returns ``torch.complex128`` ``[n_u, 2]`` in the storage order of ``u_free``.  No reference counterpart: the reference has no
mass matrix.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import require_linear
from .modal import _frozen_class
from .solve import (_AmgDevice, _REASONS, amg_host, HFEM_FLAG_PHYSICAL_GRAD, ST_FNORM, ST_HALTED, ST_ITER, ST_REASON,
                    ST_RNORM)

F64 = torch.float64
C128 = torch.complex128


@dataclass
class HarmonicInfo:
    """Outcome of one frequency: ``residual`` is ``||r||_2`` of the COCG recursion (Hermitian norm; r is updated, not
    recomputed), ``rhs_norm`` is ``||b||_2``; ``reason``: ``"rtol"``, ``"atol"``, ``"max_iter"`` or ``"breakdown"`` (a non-finite
    scalar, or ``|p^T A p| = 0`` or ``|r^T z| = 0`` before ``x`` moves: the response keeps the last good iterate)."""
    omega: float
    iterations: int
    converged: bool
    reason: str
    residual: float
    rhs_norm: float


def _check_harmonic(density, mass, rayleigh, structural, precond, precond_rebuild, rtol, atol, iters_per_graph):
    if mass not in ("consistent", "lumped"):
        raise ValueError("mass must be 'consistent' or 'lumped'")
    if precond not in ("amg", "block_jacobi", "none"):
        raise ValueError("precond must be 'amg', 'block_jacobi' or 'none'")
    if precond_rebuild not in ("each", "first"):
        raise ValueError("precond_rebuild must be 'each' or 'first'")
    density, structural = float(density), float(structural)
    alpha_r, beta_r = (float(c) for c in rayleigh)
    if not density > 0.0:
        raise ValueError("density must be > 0")
    if not (alpha_r >= 0.0 and beta_r >= 0.0 and math.isfinite(alpha_r) and math.isfinite(beta_r)):
        raise ValueError("the Rayleigh coefficients (alpha_R, beta_R) must be finite and >= 0")
    if not (structural >= 0.0 and math.isfinite(structural)):
        raise ValueError("the structural damping factor eta must be finite and >= 0")
    if int(iters_per_graph) < 1:
        raise ValueError("iters_per_graph must be >= 1")
    if rtol < 0 or atol < 0:
        raise ValueError("rtol and atol must be >= 0")
    return density, alpha_r, beta_r, structural


def _check_omega(omega) -> float:
    omega = float(omega)
    if not (math.isfinite(omega) and omega >= 0.0):
        raise ValueError("omega must be finite and >= 0")
    return omega


class HarmonicSolver:
    """Steady-state response to a harmonic load for a TRI3 or QUAD4 mesh model with an ``EnergyLoss2D`` (see the module
    docstring).

    ``density`` > 0; ``mass``: ``"consistent"`` or ``"lumped"``; ``rayleigh`` = ``(alpha_R, beta_R)``, both >= 0; ``structural``:
    the loss factor eta >= 0 of ``i eta K``; ``precond``: ``"amg"`` (a hierarchy on ``K + omega_p^2 rho M``; needs Dirichlet
    rows), ``"block_jacobi"`` (its 2x2 diagonal blocks) or ``"none"``; ``precond_rebuild``: ``"each"`` builds the preconditioner
    at every new frequency (``omega_p = omega``), ``"first"`` keeps the one of the first frequency solved after a refresh;
    stopping test ``||r||_2 <= max(rtol ||b||_2, atol)``; ``max_iter`` None = ``max(1000, 4 x free rows)``; ``iters_per_graph``:
    COCG iterations per graph replay (iterations behind the one that stopped do nothing on the device); ``b_force`` /
    ``t_force``: the callables ``loss_fn(model, b_force, t_force)`` would take.

    ``solve(omega, b=None, x0=None)`` -> ``(u_hat, HarmonicInfo)``: ``u_hat`` is ``torch.complex128`` ``[n_u, 2]`` in storage
    order; ``b`` defaults to the loss's load vector ``b0 = -dE/du(u_free = 0)`` (real: forces and the ``u_fixed`` term), or a
    real or complex ``[n_u, 2]`` tensor; ``x0``: a start (default 0).  ``sweep(omegas, rows=None, callback=None)`` solves the
    frequencies in order, each warm-started from the previous response, and returns ``(responses [n_omega, n_u, 2] -- or only
    ``rows`` of them -- , [HarmonicInfo])``.  ``operator_apply(p, omega)`` and ``assemble_operator(omega)`` are for tests and
    measurements.  Nothing of the model changes.  ``solve()`` refreshes by the frozen solver's state key when the coordinate
    rows or ``u_fixed`` moved (``refresh()`` by hand after the force callables changed).

    It owns a ``FrozenMeshSolver`` / ``Quad4FrozenMeshSolver`` (``b0``, the refresh bookkeeping and the force tables), a
    harmonic handle on the same tile plan and, for ``"block_jacobi"``, a second PCG handle that forms the blocks.  Refuses
    non-linear losses, ``EnergyLoss2D(deterministic=True)``, CPU models and a tile plan whose tiles need more than 64 KiB of LDS
    in the complex apply (``ValueError`` naming ``tile_elems``).  Not bitwise reproducible: the apply's LDS atomics carry
    last-bit noise.  COCG has no minimisation property: the residual norm is not monotone, and close to an undamped resonance
    the iteration can break down (``reason == "breakdown"``).

    THE NUMBERS ARE PHYSICAL ONLY WITH ``grad_convention="physical"`` (as ``ModalSolver`` and ``NewmarkSolver``).  ``K`` and
    ``b0`` are those of the energy ``loss_fn`` computes, so a TRI3 loss with the default ``gauss_order=4`` carries the
    reference's factor 1/2 on both."""

    def __init__(self, model, loss_fn, density: float = 1.0, mass: str = "consistent", rayleigh=(0.0, 0.0),
                 structural: float = 0.0, precond: str = "amg", precond_rebuild: str = "each", rtol: float = 1e-8,
                 atol: float = 0.0, max_iter: Optional[int] = None, iters_per_graph: int = 16,
                 b_force: Optional[Callable] = None, t_force: Optional[Callable] = None):
        require_linear(loss_fn, "HarmonicSolver")
        npe = getattr(model, "nodes_per_element", 3)
        if npe not in (3, 4) or not hasattr(model, "_conn32"):
            raise NotImplementedError("HarmonicSolver: TRI3 and QUAD4 mesh models")
        density, alpha_r, beta_r, eta = _check_harmonic(density, mass, rayleigh, structural, precond, precond_rebuild, rtol, atol,
                                                        iters_per_graph)
        if precond == "amg" and int(model._idx_udir.shape[0]) == 0:
            raise ValueError("precond='amg' needs Dirichlet rows (rigid-body modes are out of scope)")
        cls = _frozen_class(npe)
        # refuses deterministic=True and a CPU model: there is no CPU fallback
        self.solver = cls(model, loss_fn, b_force=b_force, t_force=t_force, precond="none")
        self.model, self.loss_fn, self.npe = model, loss_fn, npe
        self.density, self.mass, self.alpha_r, self.beta_r, self.eta = density, mass, alpha_r, beta_r, eta
        self.precond, self.precond_rebuild = precond, precond_rebuild
        self.rtol, self.atol, self.iters_per_graph = float(rtol), float(atol), int(iters_per_graph)
        self.lumped = mass == "lumped"
        self.device = dev = self.solver.device
        self.phys = self.solver.phys
        self.n_u = n_u = self.solver.n_u
        self.len = 4 * n_u
        self.max_iter = max(1000, 4 * n_u) if max_iter is None else int(max_iter)
        flags = HFEM_FLAG_PHYSICAL_GRAD if self.phys else 0
        h = C.c_void_p()
        rc = _lib.lib().hfem_harm_create(self.solver.plan.handle, n_u, flags, C.byref(h))
        if rc != 0:
            msg = (_lib.lib().hfem_last_error() or b"?").decode()
            if "64 KiB" in msg:
                raise ValueError(f"HarmonicSolver: the tile plan of tile_elems={loss_fn.tile_elems} does not fit the complex "
                                 f"apply ({msg}); use a loss with a smaller tile_elems")
            check(rc, "hfem_harm_create")
        self._h = h
        self._hd = None                                   # block_jacobi: the PCG handle whose shifted setup forms the blocks
        if precond == "block_jacobi":
            hd = C.c_void_p()
            check(_lib.lib().hfem_cg_create(self.solver.plan.handle, n_u, flags, C.byref(hd)), "hfem_cg_create")
            self._hd = hd
        self._amg = _AmgDevice(amg_host(model), dev, self.phys) if precond == "amg" else None
        z = dict(dtype=F64, device=dev)
        self._x = torch.zeros((2, n_u, 2), **z)           # the iterate: the captured graph only ever sees this address
        self._b = torch.zeros((2, n_u, 2), **z)
        self._x0 = torch.zeros((2, n_u, 2), **z)
        self._b0 = torch.zeros((n_u, 2), **z)
        self.diag = torch.empty((n_u, 3), **z)            # the 2x2 diagonal blocks of K + omega_p^2 rho M (block_jacobi)
        self._status = (C.c_double * 16)()
        self._graph = None
        self._key = None
        self._bound = None                                # omega the harmonic handle's coefficients are set for
        self._omega_p = None                              # omega the preconditioner was built at; None: not built

    def __del__(self):
        _lib.destroy_handle(self, "hfem_harm_destroy")
        hd = getattr(self, "_hd", None)
        if hd is not None and hd.value:
            try:
                _lib.lib().hfem_cg_destroy(hd)
            except Exception:       # interpreter shutdown: the library may already be gone
                pass
            self._hd = None

    # ---- operator and preconditioner
    def coefficients(self, omega: float):
        """``(z_K, z_M)`` as Python complex numbers; ``z_M`` includes the density."""
        omega = _check_omega(omega)
        return (complex(1.0, omega * self.beta_r + self.eta),
                complex(-self.density * omega * omega, self.density * omega * self.alpha_r))

    def _mat(self):
        return (C.c_double * 4)(*self.loss_fn._mat), float(self.loss_fn._W)

    def _bind(self, omega, coefficients=None):
        s = self.solver
        mat, W = self._mat()
        if coefficients is None:
            zk, zm = self.coefficients(omega)
        else:
            zk, zm = complex(coefficients[0]), complex(coefficients[1]) * self.density
        check(_lib.lib().hfem_harm_setup(self._h, ptr(s._xf), ptr(s._xfix) if s._xfix.numel() else None, mat, W,
                                         (C.c_double * 2)(zk.real, zk.imag), (C.c_double * 2)(zm.real, zm.imag),
                                         1 if self.lumped else 0, stream_ptr(self.device)), "hfem_harm_setup")
        self._bound = omega if coefficients is None else None

    def _build_precond(self, omega):
        """T ~ (K + omega^2 rho M)^-1: the hierarchy or the blocks, unless ``precond_rebuild="first"`` has one already."""
        if self.precond == "none" or self._omega_p == omega or (self._omega_p is not None and self.precond_rebuild == "first"):
            return
        s = self.solver
        mat, W = self._mat()
        c_m = omega * omega * self.density
        xfix = ptr(s._xfix) if s._xfix.numel() else None
        if self._amg is not None:
            self._amg.setup_shifted(s._xf, s._xfix, mat, W, 1.0, c_m, self.lumped)
        else:
            check(_lib.lib().hfem_cg_setup_shifted(self._hd, ptr(s._xf), xfix, mat, W, 1.0, c_m, 1 if self.lumped else 0, 1,
                                                   ptr(self.diag), stream_ptr(self.device)), "hfem_cg_setup_shifted")
        self._omega_p = omega

    def refresh(self):
        """Coordinates, ``u_fixed`` or the forces changed: the frozen solver's refresh, then ``b0``; the operator and the
        preconditioner are rebuilt at the next frequency."""
        s = self.solver
        s.refresh()
        with torch.no_grad():
            s._gradient(s._zero, self._b0)
            self._b0.neg_()
        self._bound = None
        self._omega_p = None
        self._key = s._state_key()

    def _ensure(self):
        if self._key is None or self._key != self.solver._state_key():
            self.refresh()

    def _planes(self, v, name):
        """A real or complex ``[n_u, 2]`` tensor as the device layout ``[2, n_u, 2]`` fp64."""
        v = v.detach()
        if tuple(v.shape) != (self.n_u, 2):
            raise ValueError(f"{name}: a real or complex tensor [{self.n_u}, 2] in the storage order of u_free")
        out = torch.zeros((2, self.n_u, 2), dtype=F64, device=self.device)
        if v.is_complex():
            v = v.to(device=self.device, dtype=C128)
            out[0].copy_(v.real)
            out[1].copy_(v.imag)
        else:
            out[0].copy_(v.to(device=self.device, dtype=F64))
        return out

    @staticmethod
    def _complex(planes):
        return torch.complex(planes[0], planes[1])

    def operator_apply(self, p: torch.Tensor, omega: Optional[float] = None, coefficients=None):
        """Standalone ``q = A p`` (complex128 ``[n_u, 2]``) and the UNCONJUGATED ``p^T A p`` (0-d complex128 device tensor);
        ``p``: a real or complex ``[n_u, 2]`` tensor in storage order.  ``A = A(omega)``, or with ``coefficients = (z_K, z_M)``
        (Python complex) the operator ``z_K K + z_M rho M``.  For tests and measurements."""
        if (omega is None) == (coefficients is None):
            raise ValueError("operator_apply: give omega or coefficients, not both")
        self._ensure()
        if coefficients is not None:
            self._bind(None, coefficients)
        else:
            omega = _check_omega(omega)
            if self._bound != omega:
                self._bind(omega)
        P = self._planes(p, "p")
        Q = torch.empty_like(P)
        pq = torch.empty(2, dtype=F64, device=self.device)
        check(_lib.lib().hfem_harm_apply(self._h, ptr(P), ptr(Q), self.len, ptr(pq), stream_ptr(self.device)), "hfem_harm_apply")
        return self._complex(Q), torch.complex(pq[0], pq[1])

    def precondition(self, r: torch.Tensor, omega: float) -> torch.Tensor:
        """``z = T r`` on one REAL plane (fp64 ``[n_u, 2]``) with the preconditioner a solve at ``omega`` uses: one V-cycle,
        ``hfem_block_jacobi_apply`` on the blocks, or a copy.  For tests and measurements."""
        omega = _check_omega(omega)
        self._ensure()
        self._build_precond(omega)
        r = _lib.require_gpu_tensor(r.detach().contiguous(), "r", F64)
        if tuple(r.shape) != (self.n_u, 2):
            raise ValueError(f"r: a real tensor [{self.n_u}, 2] in the storage order of u_free")
        if self.precond == "none":
            return r.clone()
        z = torch.empty_like(r)
        if self._amg is not None:
            check(_lib.lib().hfem_amg_vcycle(self._amg._h, ptr(r), ptr(z), stream_ptr(self.device)), "hfem_amg_vcycle")
        else:
            check(_lib.lib().hfem_block_jacobi_apply(_lib.dev_index(self.device), ptr(self.diag), ptr(r), 1, 2 * self.n_u, ptr(z),
                                                     stream_ptr(self.device)), "hfem_block_jacobi_apply")
        return z

    def assemble_operator(self, omega: float) -> torch.Tensor:
        """``A(omega)`` at the current coordinates: a complex128 ``torch.sparse_bsr_tensor`` with 2x2 blocks over the free u
        rows in storage order, composed from the real assemblies of ``K`` and ``M`` (``hfem_amg_assemble_shifted`` at (1, 0)
        and (0, 1): one thread per row, bit-deterministic)."""
        omega = _check_omega(omega)
        self._ensure()
        host = amg_host(self.model)
        a = _AmgDevice(host, self.device, self.phys)
        s = self.solver
        mat, W = self._mat()
        a.assemble_shifted(s._xf, s._xfix, mat, W, 1.0, 0.0, self.lumped)
        k = a.values(0, 0).view(-1, 2, 2).clone()
        a.assemble_shifted(s._xf, s._xfix, mat, W, 0.0, 1.0, self.lumped)
        m = a.values(0, 0).view(-1, 2, 2).clone()
        zk, zm = self.coefficients(omega)
        vals = zk * k.to(C128) + zm * m.to(C128)
        n = host.levels[0][0]
        i64 = dict(dtype=torch.int64, device=self.device)
        crow = torch.as_tensor(host.array(0, 0), **i64)
        col = torch.as_tensor(host.array(0, 1), **i64)
        return torch.sparse_bsr_tensor(crow, col, vals, size=(2 * n, 2 * n))

    # ---- one solve
    def _read_status(self):
        check(_lib.lib().hfem_harm_status(self._h, self._status, stream_ptr(self.device)), "hfem_harm_status")
        return list(self._status)

    def _iterate(self):
        """Enqueue ``iters_per_graph`` iterations on ``self._x`` (launches only: capturable)."""
        check(_lib.lib().hfem_harm_iterate(self._h, self._amg._h if self._amg is not None else None, ptr(self._x), self.len,
                                           self.iters_per_graph, stream_ptr(self.device)), "hfem_harm_iterate")

    def _replay(self):
        # the coefficients live in device memory and every pointer is the solver's own: one graph serves every frequency
        if self._graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                        # captured, not executed
                self._iterate()
            self._graph = g
        self._graph.replay()

    def _solve_planes(self, omega, warm, graph=True):
        """``self._x`` <- the response to ``self._b`` at ``omega``, started from ``self._x`` when ``warm`` (else from 0)."""
        if self._bound != omega:
            self._bind(omega)
        self._build_precond(omega)
        lib, s = _lib.lib(), stream_ptr(self.device)
        if warm:
            self._x0.copy_(self._x)
        else:
            self._x.zero_()
        check(lib.hfem_harm_start(self._h, self._amg._h if self._amg is not None else None,
                                  ptr(self.diag) if self.precond == "block_jacobi" else None, ptr(self._b),
                                  ptr(self._x0) if warm else None, self.len, self.rtol, self.atol, self.max_iter, s),
              "hfem_harm_start")
        st = self._read_status()
        while not st[ST_HALTED] and st[ST_ITER] < self.max_iter:
            if graph:
                self._replay()
            else:
                self._iterate()
            st = self._read_status()
        reason = _REASONS.get(int(st[ST_REASON]), "max_iter")
        return HarmonicInfo(omega=omega, iterations=int(st[ST_ITER]), converged=reason in ("rtol", "atol"), reason=reason,
                            residual=float(st[ST_RNORM]), rhs_norm=float(st[ST_FNORM]))

    def _set_rhs(self, b):
        if b is None:
            self._b.zero_()
            self._b[0].copy_(self._b0)
        else:
            self._b.copy_(self._planes(b, "b"))

    def solve(self, omega: float, b: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None, graph: bool = True):
        """The response at one frequency -> ``(u_hat, HarmonicInfo)`` (see the class docstring).  ``graph=False`` enqueues the
        iterations directly instead of replaying the captured graph (for tests)."""
        omega = _check_omega(omega)
        self._ensure()
        with torch.no_grad():
            self._set_rhs(b)
            if x0 is not None:
                self._x.copy_(self._planes(x0, "x0"))
            info = self._solve_planes(omega, warm=x0 is not None, graph=graph)
            return self._complex(self._x), info

    def sweep(self, omegas, rows=None, callback: Optional[Callable] = None):
        """The responses to ``b0`` at ``omegas`` in the order given, each warm-started from the previous one.  Returns
        ``(responses, [HarmonicInfo])``: complex128 ``[n_omega, n_u, 2]``, or ``[n_omega, len(rows), 2]`` when ``rows`` (an index
        tensor or list of free u rows) is given.  ``callback(omega, u_hat, info)`` after every frequency."""
        omegas = [_check_omega(w) for w in omegas]
        self._ensure()
        idx = None if rows is None else torch.as_tensor(rows, dtype=torch.int64, device=self.device)
        n_out = self.n_u if idx is None else int(idx.shape[0])
        out = torch.zeros((len(omegas), n_out, 2), dtype=C128, device=self.device)
        infos = []
        with torch.no_grad():
            self._set_rhs(None)
            for i, w in enumerate(omegas):
                info = self._solve_planes(w, warm=i > 0)
                u = self._complex(self._x)
                out[i].copy_(u if idx is None else u[idx])
                infos.append(info)
                if callback is not None:
                    callback(w, u, info)
        return out, infos


def frequency_response(model, loss_fn, omegas, rows=None, callback: Optional[Callable] = None, **kw):
    """One-shot ``HarmonicSolver(model, loss_fn, **kw).sweep(omegas, rows, callback)``."""
    return HarmonicSolver(model, loss_fn, **kw).sweep(omegas, rows=rows, callback=callback)
