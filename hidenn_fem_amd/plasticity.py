"""Small-strain J2 elastoplasticity of a TRI3 model in plane strain: load paths by Newton-Krylov on the consistent tangent
(DESIGN 31).

Rate-independent J2 plasticity with linear isotropic hardening has a closed-form radial return and an incremental potential
``Psi(eps; eps^p_n, alpha_n)`` whose gradient is the stress and whose Hessian is the consistent tangent, so one load step is
the minimisation of ``Pi(u) = sum_e A_e Psi_e(eps(u)) - load f_ext . u`` over ``u_free`` against the COMMITTED state: the
inexact Newton of ``hidenn_fem_amd.newton._NewtonSolverBase`` (Eisenstat-Walker forcing, Armijo backtracking on ``Pi``, truncated
PCG on the tangent) carries over with two launches replaced --

* the update launch (``csrc/tri3_j2.hip``): strain, return map against the committed state by element id, internal force and
  ``Pi`` in one launch on the one-element-per-slot plan; the external load is ``load * g_ext`` added on write-out, ``g_ext``
  formed once per refresh by the linear energy launch at ``u = 0``;
* the linearisation launch: the same return map at the Newton iterate, one tangent record ``{theta, theta_bar, n}`` per slot of
  the plan and the block-Jacobi blocks.  The tangent apply of every CG iteration reads coordinates, ``p`` and those records only.

TRI3 has constant strain: one state point per element, ``{eps^p_xx, eps^p_yy, eps^p_xy, alpha}``.

Not deterministic in the last bits (LDS atomics), but state and stress are functions of ``u`` alone, element by element.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import EnergyLoss2D
from .newton import NewtonInfo, _NewtonSolverBase
from .solve import F64, HFEM_FLAG_NO_EDGES, HFEM_FLAG_NO_GX, _Frozen


class J2PlasticityLoss2D(EnergyLoss2D):
    """Material and force description of small-strain J2 plasticity with linear isotropic hardening, plane strain, for TRI3
    models: ``mu = E / (2 (1 + nu))``, ``lambda = E nu / ((1 + nu)(1 - 2 nu))`` (``loss_fn.lame = (lambda, mu)``),
    ``kappa = lambda + 2 mu / 3``, yield stress ``sigma_y > 0``, hardening modulus ``hardening >= 0``.  The force tables (body
    force at the reference Gauss points, tractions) are ``EnergyLoss2D``'s; ``grad_convention`` is always ``"physical"``.

    It is NOT callable as a loss: the potential is incremental and means nothing without a committed state -- that state lives
    in ``ElastoplasticSolver`` (``elastoplastic_solve_``), which takes this object.  Not available: ``deterministic=True``,
    ``arithmetic="fp32"`` (fp32 models: rows widened once, fp64 arithmetic), QUAD4 models, the linear tools and the
    finite-strain solvers."""

    elastoplastic = True

    def __init__(self, E: float = 10e9, nu: float = 0.3, sigma_y: float = 1e5, hardening: float = 0.0, length: float = 1.0,
                 height: float = 1.0, gauss_order: int = 4, gauss_order_1d: int = 2, device: Optional[torch.device] = None,
                 dtype: torch.dtype = torch.float32, tile_elems: int = 0, deterministic: bool = False,
                 arithmetic: str = "auto"):
        if not (math.isfinite(sigma_y) and sigma_y > 0.0):
            raise ValueError("J2PlasticityLoss2D: sigma_y must be finite and > 0")
        if not (math.isfinite(hardening) and hardening >= 0.0):
            raise ValueError("J2PlasticityLoss2D: hardening must be finite and >= 0")
        if deterministic:
            raise NotImplementedError("J2PlasticityLoss2D: no fixed-order kernel (deterministic=True) for this material")
        if arithmetic == "fp32":
            raise NotImplementedError("J2PlasticityLoss2D: fp64 arithmetic only (fp32 models: float rows, fp64 arithmetic)")
        super().__init__(E, nu, length, height, gauss_order, gauss_order_1d, device, dtype, tile_elems,
                         grad_convention="physical", deterministic=False, arithmetic=arithmetic)
        self.plane = "strain"
        self.sigma_y, self.hardening = float(sigma_y), float(hardening)
        mu = E / (2.0 * (1.0 + nu))
        lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
        self.lame = (lam, mu)
        self.kappa = lam + 2.0 * mu / 3.0

    @staticmethod
    def require_tri3(model, who: str):
        if getattr(model, "nodes_per_element", 3) != 3:
            raise NotImplementedError(f"{who}: TRI3 models only (QUAD4 needs four state points per cell: not built yet)")

    def _refuse(self, *a, **k):
        raise NotImplementedError("J2PlasticityLoss2D is not a loss to call: its potential is incremental and needs a committed "
                                  "state -- use hidenn_fem_amd.plasticity.ElastoplasticSolver / elastoplastic_solve_")

    __call__ = domain_energy = value_and_grad_ = _refuse


class ElastoplasticSolver(_NewtonSolverBase):
    """Load stepping of a TRI3 model under a ``J2PlasticityLoss2D`` at its CURRENT coordinates.

    ``solve(load=1.0, commit=True)`` minimises the incremental potential of ONE load step over ``u_free`` from the current
    ``model.u_free`` against the committed state, writes the result into ``model.u_free`` and returns a ``NewtonInfo``
    (``min_J`` is 1: small strain).  ``load`` scales the external forces (``b_force`` / ``t_force``, tabulated as the loss does)
    AND the Dirichlet values ``u_fixed`` (in a solver-owned buffer: displacement control; ``model.u_fixed`` is not written).
    With ``commit`` the trial state of the returned ``u`` becomes the committed one.  ``run(loads)`` takes the steps in
    order.  ``reset()`` returns to the virgin state.  ``state()`` -> ``(eps_p [ne, 3], alpha [ne])`` committed,
    ``stress()`` -> ``[ne, 4] = (s_xx, s_yy, s_xy, s_zz)`` and ``von_mises()`` -> ``[ne]`` of the last update launch, all in
    the model's element order; ``plastic_fraction``: the share of elements that yielded in the last solve's final state.

    Loop, forcing, line search, preconditioners (``"block_jacobi"``, ``"none"``, ``"amg"``: the small-strain hierarchy with
    the elastic moduli, a fixed SPD preconditioner for the softening tangent), graph replay and every keyword are
    ``_NewtonSolverBase``'s; ``||g(u_free = 0)||`` of the stopping test is taken at the step's load and committed state."""

    def __init__(self, model, loss_fn, b_force: Optional[Callable] = None, t_force: Optional[Callable] = None,
                 precond: str = "block_jacobi", rtol: float = 1e-8, atol: float = 0.0, max_newton: int = 50,
                 cg_max_iter: Optional[int] = None, iters_per_graph: int = 16, eta_max: float = 0.1, armijo: float = 1e-4,
                 max_backtracks: int = 30):
        if precond not in ("block_jacobi", "none", "amg"):
            raise ValueError("precond must be 'block_jacobi', 'none' or 'amg'")
        super().__init__(model, loss_fn, b_force, t_force, precond, rtol, atol, max_newton, cg_max_iter, iters_per_graph,
                         eta_max, armijo, max_backtracks)
        dev, z = self.device, dict(dtype=F64, device=self.device)
        self.ne = int(model.connectivity.shape[0])
        lam, mu = loss_fn.lame
        j = C.c_void_p()
        check(_lib.lib().hfem_j2_create(self.plan.handle, self.ne, (C.c_double * 4)(mu, loss_fn.kappa, loss_fn.sigma_y,
                                                                                   loss_fn.hardening),
                                        float(loss_fn._W), C.byref(j)), "hfem_j2_create")
        self._j2 = j
        self._tan = torch.zeros(max(int(_lib.lib().hfem_j2_slots(j)), 1), **z)
        self._ufix0 = torch.zeros_like(self._ufix)     # the Dirichlet values at load 1
        self._gext = torch.zeros((self.n_u, 2), **z)
        self._pi = torch.zeros(3, **z)                 # {Pi, plastic count, max dgamma} of the last update launch
        self._plinfo = torch.zeros(2, **z)             # {plastic count, 0} of the last linearisation
        self._out[1] = 1.0                             # the base reads {Pi, min J, inverted}: small strain has no J
        self._info[0] = 1.0
        self._load = 1.0
        self._write = 0
        self._loss0 = torch.zeros((), **z)

    def __del__(self):
        h = getattr(self, "_j2", None)
        if h is not None and h.value:
            try:
                _lib.lib().hfem_j2_destroy(h)
            except Exception:
                pass
            self._j2 = None
        super().__del__()

    @staticmethod
    def _check_model(model, loss_fn):
        if not isinstance(loss_fn, J2PlasticityLoss2D):
            raise NotImplementedError("ElastoplasticSolver: J2PlasticityLoss2D only (an EnergyLoss2D: FrozenMeshSolver; a "
                                      "NeoHookeanLoss2D: NewtonKrylovSolver)")
        J2PlasticityLoss2D.require_tri3(model, "ElastoplasticSolver")

    @staticmethod
    def _make_plan(model, loss_fn):
        from .plan import model_plan
        return model_plan(model, loss_fn.tile_elems, paired=False)

    def _body(self):
        return (C.c_double * 6)(*self.loss_fn._body_table(self.b_force))

    # ---- refresh: rows, the AMG numbers and g_ext = the linear energy's gradient at u = 0 with zero Dirichlet values
    def refresh(self):
        m, lf, dev = self.model, self.loss_fn, self.device
        with torch.no_grad():
            self._xf.copy_(m.node_coords_free.detach())
            self._xfix.copy_(m.node_coords_fixed.detach())
            self._ufix0.copy_(m.u_fixed_rows().detach())
            flags = HFEM_FLAG_NO_GX                      # at u = 0 the gradient is the load vector in either convention
            if m.neumann_edges is None or m.N_edges == 0:
                te, tc, flags = None, [0.0] * 4, flags | HFEM_FLAG_NO_EDGES
            else:
                te, tc = lf._traction(_Frozen(m, self._xf, self._xfix), self.t_force)
                te = None if te is None else te.to(device=dev, dtype=F64).contiguous()
            self._tables = (self._body(), te, None if tc is None else (C.c_double * 4)(*tc), flags)
            if self._amg is not None:
                self._small_strain_setup()
            zero_fix = torch.zeros_like(self._ufix0)
            check(_lib.lib().hfem_tri3_energy_plan(
                self.plan.handle, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(self._zero),
                ptr(zero_fix) if zero_fix.numel() else None, (C.c_double * 4)(*lf._mat), float(lf._W), self._tables[0], ptr(te),
                self._tables[2], 0, -1, ptr(self._loss0), None, ptr(self._gext), flags, stream_ptr(dev)),
                "hfem_tri3_energy_plan")
            self._set_load(self._load)
        self._key = self._state_key()

    def _set_load(self, load: float):
        self._load = float(load)
        torch.mul(self._ufix0, self._load, out=self._ufix)
        self._energy(self._zero, self._gz)
        self._rhs_norm = float(torch.linalg.vector_norm(self._gz))

    # ---- launches
    def _energy(self, u, g, tables=None):
        check(_lib.lib().hfem_j2_update(
            self._j2, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(u),
            ptr(self._ufix) if self._ufix.numel() else None, ptr(self._gext), self._load, self._write, ptr(self._pi), ptr(g),
            stream_ptr(self.device)), "hfem_j2_update")
        self._out[0:1].copy_(self._pi[0:1])

    def _linearise(self):
        check(_lib.lib().hfem_cg_setup_j2(
            self._h, self._j2, ptr(self._xf), ptr(self._xfix) if self._xfix.numel() else None, ptr(self._u),
            ptr(self._ufix) if self._ufix.numel() else None, ptr(self._tan), 1 if self.precond == "block_jacobi" else 0,
            ptr(self.diag), ptr(self._plinfo), stream_ptr(self.device)), "hfem_cg_setup_j2")

    # ---- the load path
    def solve(self, load: float = 1.0, commit: bool = True) -> NewtonInfo:
        if not math.isfinite(load):
            raise ValueError("load must be finite")
        self._fresh()
        with torch.no_grad():
            self._set_load(load)
        info = super().solve()
        with torch.no_grad():                            # the trial state and the stress of the returned u
            self._write = 1
            try:
                self._energy(self._u, self._gt)
            finally:
                self._write = 0
            self._last = self._pi.tolist()
            if commit:
                check(_lib.lib().hfem_j2_commit(self._j2, stream_ptr(self.device)), "hfem_j2_commit")
        return info

    def run(self, loads: Sequence[float]) -> List[NewtonInfo]:
        return [self.solve(float(l)) for l in loads]

    def reset(self):
        """The virgin state: no plastic strain, no hardening."""
        check(_lib.lib().hfem_j2_set(self._j2, None, stream_ptr(self.device)), "hfem_j2_set")
        self._last = [0.0, 0.0, 0.0]

    def _get(self, which):
        out = torch.empty((self.ne, 4), dtype=F64, device=self.device)
        check(_lib.lib().hfem_j2_get(self._j2, which, ptr(out), stream_ptr(self.device)), "hfem_j2_get")
        return out

    def state(self, trial: bool = False):
        """``(eps_p [ne, 3], alpha [ne])`` of the committed state (``trial=True``: of the last solve's trial state)."""
        s = self._get(1 if trial else 0)
        return s[:, :3].contiguous(), s[:, 3].contiguous()

    def set_state(self, eps_p: torch.Tensor, alpha: torch.Tensor):
        """Committed = trial = the given state (a test helper), ``[ne, 3]`` and ``[ne]`` in the model's element order."""
        s = torch.cat([eps_p.detach().to(device=self.device, dtype=F64).reshape(self.ne, 3),
                       alpha.detach().to(device=self.device, dtype=F64).reshape(self.ne, 1)], dim=1).contiguous()
        check(_lib.lib().hfem_j2_set(self._j2, ptr(s), stream_ptr(self.device)), "hfem_j2_set")

    def stress(self) -> torch.Tensor:
        return self._get(2)

    def von_mises(self) -> torch.Tensor:
        s = self._get(2)
        p = (s[:, 0] + s[:, 1] + s[:, 3]) / 3.0
        d = torch.stack([s[:, 0] - p, s[:, 1] - p, s[:, 3] - p], dim=1)
        return torch.sqrt(1.5 * ((d * d).sum(dim=1) + 2.0 * s[:, 2] ** 2))

    @property
    def plastic_fraction(self) -> float:
        return float(getattr(self, "_last", [0.0, 0.0, 0.0])[1]) / max(self.ne, 1)

    @property
    def max_dgamma(self) -> float:
        return float(getattr(self, "_last", [0.0, 0.0, 0.0])[2])

    @property
    def info(self) -> torch.Tensor:
        """``{plastic element count, 0}`` of the last linearisation (fp64 device tensor, the same every call)."""
        return self._plinfo

    # ---- test helpers
    def evaluate(self, write: bool = True):
        """One update launch at the current ``model.u_free`` and load: -> ``(out [3] = {Pi, plastic count, max dgamma},
        g [n_u, 2])``; with ``write`` the trial state and the stress follow."""
        self._fresh()
        with torch.no_grad():
            self._u.copy_(self.model.u_free.detach())
            self._write = 1 if write else 0
            try:
                self._energy(self._u, self._g)
            finally:
                self._write = 0
        return self._pi.clone(), self._g.clone()

    def commit(self):
        check(_lib.lib().hfem_j2_commit(self._j2, stream_ptr(self.device)), "hfem_j2_commit")


def elastoplastic_solve_(model, loss_fn, loads: Sequence[float], **kw) -> List[NewtonInfo]:
    """One-shot ``ElastoplasticSolver(model, loss_fn, **kw).run(loads)`` from the virgin state: ``model.u_free`` ends at the
    last load's equilibrium (in place)."""
    return ElastoplasticSolver(model, loss_fn, **kw).run(loads)
