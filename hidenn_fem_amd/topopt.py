"""Density-based (SIMP) compliance topology optimisation on a frozen mesh, TRI3 and QUAD4.

    minimise    c(rho) = f^T u = u^T K(w) u,   K(w) u = f,   K(w) = sum_e w_e K_e,   w_e = e_min + rho~_e^penal (1 - e_min)
    subject to  sum_e v_e rho~_e <= volume_fraction sum_e v_e,   0 <= rho_e <= 1,   rho~ = F rho  (linear density filter)

One design iteration (``TopologyOptimizer.step``) is, in order: the weights launch (``hfem_topt_weights``), the numeric AMG
setup on ``K(w)`` or its 2x2 blocks (``hfem_amg_setup_scaled`` / ``hfem_cg_setup_scaled``), a warm-started PCG solve through
the ``Scaled`` instances of the plain element kernels, one launch for the element energies ``ce_e = u_e^T K_e u_e`` and
``dc/drho~_e = -penal rho~_e^(penal-1) (1 - e_min) ce_e`` (``hfem_topt_energy``), the transpose filter ``dc/drho = F^T dc/drho~``
and the optimality-criteria update with its bisection on the device (``hfem_topt_oc``: launches only; the host reads one status
record per iteration).  The PCG driver, the AMG hierarchy (patterns and aggregates are the mesh's; only values are rebuilt) and
the graph replay are ``FrozenMeshSolver``'s.

Out of scope: any update other than OC (MMA), Heaviside projection and sensitivity filtering, a scaled energy loss or stress
recovery (``loss_fn(model)`` stays homogeneous), density-dependent body forces, a scaled mass (dynamics, modes or buckling on a
design), finite strain, sharded runs and fp32 operators.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional

import torch

from .loss import require_linear
from .solve import ElementWeights, FrozenMeshSolver, Quad4FrozenMeshSolver

F64 = torch.float64


@dataclass
class TopOptInfo:
    """Outcome of one ``TopologyOptimizer.step()``: ``compliance`` ``f^T u`` of the design the step started from, ``volume``
    ``sum_e v_e rho~_e`` of the design it produced, ``change`` ``max_e |rho_new - rho|``, ``iterations`` of the PCG solve
    (``converged``: it met its tolerance), ``lam`` the multiplier at the feasible end of the final bracket, ``feasible``:
    the update met the volume target."""
    compliance: float
    volume: float
    change: float
    iterations: int
    lam: float
    feasible: bool
    converged: bool


def element_geometry(model, coords: Optional[torch.Tensor] = None):
    """(centroids fp64 ``[ne, 2]``, volumes fp64 ``[ne]``) of a TRI3 or QUAD4 model at its current coordinates (unit
    thickness: a volume is the element's area, by the shoelace formula)."""
    if coords is None:
        from . import ops
        with torch.no_grad():
            coords = ops.AssembleRowsFn.apply(model.node_coords_free.detach(), model.node_coords_fixed.detach(), model._idx_free,
                                              model._idx_fixed, model.Nnodes)
    X = coords.detach().to(F64)[model.connectivity.long()]          # [ne, npe, 2]
    Xn = torch.roll(X, -1, dims=1)
    area = 0.5 * (X[..., 0] * Xn[..., 1] - Xn[..., 0] * X[..., 1]).sum(dim=1).abs()
    return X.mean(dim=1).contiguous(), area.contiguous()


class TopologyOptimizer:
    """SIMP compliance minimisation of ``model`` (TRI3 or QUAD4) under ``loss_fn`` (an ``EnergyLoss2D``: its material and its
    forces), see the module docstring.

    ``volume_fraction`` in (0, 1]: the target ``sum v rho~ / sum v``; the design starts uniform at it.  ``penal >= 1``;
    ``filter_radius``: the density filter's radius in the mesh's length unit (None: 1.5 mean element sizes, the square root
    of the mean element volume; 0: no filter); ``e_min`` in (0, 1): the void's relative stiffness; ``move``: the OC move
    limit; ``n_bisect``: halvings of the multiplier's bracket per update; ``precond`` / ``rtol`` / ``atol`` / ``max_iter`` /
    ``iters_per_graph`` / ``b_force`` / ``t_force``: ``FrozenMeshSolver``'s.

    Refused: a finite-strain loss, ``EnergyLoss2D(deterministic=True)``, nonzero ``u_fixed`` (the Dirichlet lift comes from
    the homogeneous energy launch), ``precond="amg"`` without Dirichlet rows.  The loads are design-independent.

    ``density`` / ``filtered_density``: fp64 ``[ne]`` in the model's element order.  ``step()`` runs one design iteration and
    returns a ``TopOptInfo``; ``run(n_iter, tol)`` iterates it until ``change <= tol``; ``compliance()`` / ``sensitivity()``
    evaluate at the current design without updating it.  Of the model only ``u_free`` changes (the displacement of the last
    solve); coordinates and every ``.grad`` are untouched.  Geometry (element volumes and centroids, by torch) is taken at
    construction: the mesh is frozen for the life of the optimizer."""

    def __init__(self, model, loss_fn, volume_fraction: float, penal: float = 3.0, filter_radius: Optional[float] = None,
                 e_min: float = 1e-9, move: float = 0.2, n_bisect: int = 60, precond: str = "amg", rtol: float = 1e-8,
                 atol: float = 0.0, max_iter: Optional[int] = None, iters_per_graph: int = 16,
                 b_force: Optional[Callable] = None, t_force: Optional[Callable] = None):
        require_linear(loss_fn, "TopologyOptimizer")
        npe = getattr(model, "nodes_per_element", 3)
        if npe not in (3, 4) or not hasattr(model, "connectivity"):
            raise NotImplementedError("TopologyOptimizer: TRI3 and QUAD4 mesh models")
        if getattr(loss_fn, "deterministic", False):
            raise NotImplementedError("TopologyOptimizer: EnergyLoss2D(deterministic=True) has no solver counterpart")
        if int(model._idx_udir.shape[0]) and bool((model.u_fixed_rows().detach() != 0).any()):
            raise ValueError("TopologyOptimizer needs u_fixed == 0: the Dirichlet lift comes from the homogeneous energy launch")
        if precond == "amg" and int(model._idx_udir.shape[0]) == 0:
            raise ValueError("precond='amg' needs Dirichlet rows: without them K_ff and the coarse operator are singular")
        if not (0.0 < float(volume_fraction) <= 1.0):
            raise ValueError("volume_fraction must be in (0, 1]")
        if not (math.isfinite(penal) and penal >= 1.0):
            raise ValueError("penal must be finite and >= 1")
        if not (0.0 < float(e_min) < 1.0):
            raise ValueError("e_min must be in (0, 1)")
        if not (0.0 < float(move) <= 1.0):
            raise ValueError("move must be in (0, 1]")
        if not (1 <= int(n_bisect) <= 4096):
            raise ValueError("n_bisect must be in [1, 4096]")
        if filter_radius is not None and not (math.isfinite(filter_radius) and filter_radius >= 0.0):
            raise ValueError("filter_radius must be finite and >= 0 (None: 1.5 mean element sizes)")
        cls = Quad4FrozenMeshSolver if npe == 4 else FrozenMeshSolver
        self.solver = cls(model, loss_fn, b_force=b_force, t_force=t_force, precond=precond, rtol=rtol, atol=atol,
                          max_iter=max_iter, iters_per_graph=iters_per_graph)
        self.model, self.loss_fn = model, loss_fn
        self.volume_fraction, self.penal, self.e_min = float(volume_fraction), float(penal), float(e_min)
        self.move, self.n_bisect = float(move), int(n_bisect)
        dev = self.solver.device
        self.device = dev
        self.ne = int(model.connectivity.shape[0])
        self.centroids, self.volumes = element_geometry(model)
        self.filter_radius = 1.5 * math.sqrt(float(self.volumes.mean())) if filter_radius is None else float(filter_radius)
        self.weights = ElementWeights(self.solver.plan, self.ne, dev, centroids=self.centroids, volumes=self.volumes,
                                      radius=self.filter_radius)
        self.solver.bind_element_weights(self.weights)
        self.vol_target = self.volume_fraction * float(self.volumes.sum())
        z = dict(dtype=F64, device=dev)
        self.density = torch.full((self.ne,), self.volume_fraction, **z)
        self.filtered_density = self.weights.filter(self.density)
        self._rho_new, self._rho_f_new = torch.empty(self.ne, **z), torch.empty(self.ne, **z)
        self._ce, self._dc = torch.empty(self.ne, **z), torch.empty(self.ne, **z)
        self._dv = self.weights.filter(self.volumes, transpose=True)      # d(sum v rho~) / d rho = F^T v: the mesh's
        self.iteration = 0

    # ---- the state equation at the current design
    def _solve(self):
        s = self.solver
        self.weights.simp(self.filtered_density, self.penal, self.e_min)
        s.relinearise()                                          # new weights in the bound buffers: values only
        info = s.solve()
        self.weights.energy(*s.element_energy_inputs(), self.filtered_density, self.penal, self.e_min, self._ce, self._dc)
        return info

    def compliance(self) -> float:
        """``f^T u = sum_e w_e u_e^T K_e u_e`` at the current design (one solve; ``model.u_free`` holds its displacement)."""
        self._solve()
        return float(torch.dot(self.weights.w_elem, self._ce))

    def sensitivity(self) -> torch.Tensor:
        """``dc/drho`` (fp64 ``[ne]``) at the current design: ``F^T`` of ``-penal rho~^(penal-1) (1 - e_min) u_e^T K_e u_e``."""
        self._solve()
        return self.weights.filter(self._dc, transpose=True)

    def step(self) -> TopOptInfo:
        info = self._solve()
        c = torch.dot(self.weights.w_elem, self._ce)
        dcf = self.weights.filter(self._dc, transpose=True)
        self.weights.oc(self.density, dcf, self._dv, self.vol_target, self.move, self.n_bisect, self._rho_new, self._rho_f_new)
        change = (self._rho_new - self.density).abs().max()
        st = self.weights.status()
        self.density, self._rho_new = self._rho_new, self.density
        self.filtered_density, self._rho_f_new = self._rho_f_new, self.filtered_density
        self.iteration += 1
        return TopOptInfo(compliance=float(c), volume=float(st["volume"]), change=float(change), iterations=info.iterations,
                          lam=float(st["lambda_hi"]), feasible=bool(st["feasible"]), converged=info.converged)

    def run(self, n_iter: int, tol: float = 1e-2) -> List[TopOptInfo]:
        """Up to ``n_iter`` design iterations, stopping once ``change <= tol``."""
        out = []
        for _ in range(int(n_iter)):
            out.append(self.step())
            if out[-1].change <= tol:
                break
        return out


def minimize_compliance_(model, loss_fn, volume_fraction: float, n_iter: int = 50, tol: float = 1e-2, **kw):
    """One-shot ``TopologyOptimizer(model, loss_fn, volume_fraction, **kw).run(n_iter, tol)`` followed by one solve at the final
    design, whose displacement stays in ``model.u_free``.  Returns ``(filtered_density, infos, final_compliance)``."""
    opt = TopologyOptimizer(model, loss_fn, volume_fraction, **kw)
    infos = opt.run(n_iter, tol)
    c = opt.compliance()
    return opt.filtered_density, infos, c
