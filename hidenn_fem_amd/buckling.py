"""Linearised (eigenvalue) buckling of a TRI3 or QUAD4 model: the smallest positive load factors of
``(K + lambda K_G(sigma_0)) phi = 0`` by block LOBPCG.

With ``theta = -1 / lambda`` the problem is ``K_G phi = theta K phi``: ``K_G`` symmetric indefinite, ``K`` symmetric positive
definite, and the smallest (most negative) ``theta`` are the smallest positive load factors.  That is the problem
``ModalSolver`` iterates with the roles swapped -- ``K_G`` where the modal pencil has ``K``, ``K`` where it has ``M`` -- so
``BucklingSolver`` is that solver on another pencil: the same loop, Ritz step, Gram / combine / residual kernels and
preconditioner ``T ~ K^-1`` (csrc/modal.hip), ``K`` through ``hfem_cg_apply``, and the one new operator, the geometric stiffness
``K_G`` of the prestress ``sigma_0 = C eps(u_0)``, through ``hfem_geom_setup`` / ``hfem_geom_apply`` (csrc/buckling.hip)::

    v^T K_G v = sum_e sum_q w_q |det J_q| sum_{i in x, y} (grad v_i)^T S_0(q) (grad v_i),   S_0 = [[s_xx, s_xy], [s_xy, s_yy]]

in the gradient convention and with the quadrature of the loss (TRI3: constant gradients, weight sum ``loss_fn._W``; QUAD4: the
2x2 Gauss rule of ``K``).  No reference counterpart.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .modal import F64, MAX_BLOCK, ModalSolver
from .solve import HFEM_FLAG_PHYSICAL_GRAD


@dataclass
class BucklingInfo:
    """Outcome of ``BucklingSolver.solve()``.  ``theta`` [n_modes]: ascending eigenvalues of ``K_G x = theta K x`` (fp64, CPU);
    ``load_factors`` = ``-1 / theta`` where ``theta < 0`` and ``inf`` where ``theta >= 0`` (no buckling under this load at any
    positive factor); ``n_buckling``: how many of the returned ``theta`` are negative (a body in pure tension has none: a
    result, not an error); ``modes`` [n_modes, n_u, 2]: fp64 on the model's device, rows in the storage order of ``u_free``,
    K-orthonormal; ``residual_norms`` [n_modes]: ||K_G x_j - theta_j K x_j||_2; ``iterations``: LOBPCG iterations done;
    ``converged``: every one of the ``n_modes`` pairs met ``||K_G x - theta K x||_2 <= rtol |theta| ||K x||_2``."""
    theta: torch.Tensor
    load_factors: torch.Tensor
    n_buckling: int
    modes: torch.Tensor
    residual_norms: torch.Tensor
    iterations: int
    converged: bool


class BucklingSolver(ModalSolver):
    """Smallest ``n_modes`` positive buckling load factors of a TRI3 or QUAD4 mesh model with an ``EnergyLoss2D``, about the
    reference state ``u_0 = model.u_free`` AS IT STANDS WHEN ``solve()`` IS CALLED (widened to fp64, ``u_fixed`` of the model on
    the Dirichlet rows): a load ``lambda`` times the one that produced ``u_0`` buckles the body at ``lambda = load_factors``.

    ``precond``: ``"amg"`` (one V-cycle on K per column and iteration) or ``"block_jacobi"`` (the 2x2 diagonal blocks of K);
    ``block``: width of the iterated block, default ``min(8, n_modes + 2)``, ``1 <= n_modes <= block <= 8``; ``rtol``,
    ``max_iter``, ``seed`` as ``ModalSolver``, whose iteration this is (block LOBPCG with its Ritz step, restarts and one host
    synchronisation per iteration; in addition the ``W`` and ``P`` columns of a mode that has converged are left out of the basis
    -- soft locking --, which ``restarts`` does not count), on the pencil ``(K_G, K)``: per iteration ``K_G W`` by one ``hfem_geom_apply`` launch and
    ``K W`` by ``block`` calls of ``hfem_cg_apply``.  Mode j is converged when
    ``||K_G x_j - theta_j K x_j||_2 <= rtol |theta_j| ||K x_j||_2``.

    The element matrices of ``K_G`` (one ``hfem_geom_setup`` launch) are rebuilt when the owned frozen-mesh solver's state key
    changes (coordinates, ``u_fixed``) or when ``u_free`` changed (``data_ptr``, ``_version``).  The model, its parameters and
    every ``.grad`` are left untouched.  fp32 models are solved in fp64 on their widened rows.

    THE FACTORS ARE PHYSICAL ONLY WITH ``grad_convention="physical"`` (as the modal frequencies): in the reference convention
    the pencil is still symmetric with K positive definite and is solved the same way, but its factors are not those of the
    elastic body.  FOR TRI3 THEY ARE PHYSICAL ONLY WITH ``gauss_order=1``: the default ``gauss_order=4`` carries the reference's
    weight sum 1/4 into K and K_G alike, which leaves theta unchanged for a GIVEN ``u_0`` but doubles the ``u_0`` a static solve
    returns for a given load.  MODES FOR THE REVERSED LOAD (negative ``lambda``, positive ``theta``) ARE NOT SOUGHT: the iteration
    converges to the lowest ``theta``; where fewer than ``n_modes`` of them are negative the rest come back with
    ``load_factors = inf``.  The model needs Dirichlet rows; GPU only."""

    _who = "BucklingSolver"

    def __init__(self, model, loss_fn, n_modes: int = 4, precond: str = "amg", rtol: float = 1e-8, max_iter: int = 200,
                 block=None, seed: int = 0):
        super().__init__(model, loss_fn, n_modes=n_modes, precond=precond, rtol=rtol, max_iter=max_iter, block=block, seed=seed)
        dev = self.device
        fixed_row = torch.full((model.Nnodes,), -1, dtype=torch.int32, device=dev)
        idx_dir = model._idx_udir.to(device=dev, dtype=torch.long)
        fixed_row[idx_dir] = torch.arange(idx_dir.shape[0], dtype=torch.int32, device=dev)
        self._fixed_row = fixed_row
        self._u0 = torch.empty((self.n_u, 2), dtype=F64, device=dev)
        self._ge = torch.empty((model.Nelems, self.npe, self.npe), dtype=F64, device=dev)     # G_e, full rows
        self._geom_key = None

    # ---- the prestress
    def _prestress_key(self):
        u = self.model.u_free
        return (self.solver._state_key(), u.data_ptr(), u._version)

    def _refresh(self):
        super()._refresh()
        key = self._prestress_key()
        if self._geom_key is None or self._geom_key != key:
            md, sv = self.model, self.solver
            with torch.no_grad():
                self._u0.copy_(md.u_free.detach())
            mat = (C.c_double * 4)(*self.loss_fn._mat)
            n_fix = int(sv._ufix.shape[0])
            check(_lib.lib().hfem_geom_setup(_lib.dev_index(self.device), self.npe, HFEM_FLAG_PHYSICAL_GRAD if sv.phys else 0,
                                             ptr(self._x64), ptr(md._conn32), md.Nelems, md.Nnodes, ptr(self._u0), self.n_u,
                                             ptr(sv._ufix) if n_fix else None, n_fix, ptr(self._node_row), ptr(self._fixed_row),
                                             mat, float(self.loss_fn._W), ptr(self._ge), stream_ptr(self.device)),
                  "hfem_geom_setup")
            self._geom_key = key

    # ---- the pencil (K_G, K)
    def _geom_into(self, V, out, m):
        """out[:m] = K_G V[:m] (any m: the entry point takes at most 8 columns a call)."""
        md = self.model
        for k in range(0, m, MAX_BLOCK):
            mk = min(MAX_BLOCK, m - k)
            check(_lib.lib().hfem_geom_apply(_lib.dev_index(self.device), self.npe, ptr(self._ge), ptr(md._conn32), md.Nelems,
                                             md.Nnodes, ptr(self._adj_ptr), ptr(self._adj), ptr(self._row_node),
                                             ptr(self._node_row), self.n_u, ptr(V[k]), mk, ptr(out[k]), stream_ptr(self.device)),
                  "hfem_geom_apply")

    def _a_into(self, V, out, m):
        self._geom_into(V, out, m)

    def _b_into(self, V, out, m):
        self._stiffness_into(V, out, m)

    def _ritz_order(self, b, at, ms, norms, lam):
        """X, then W and P of the columns that have NOT met the convergence criterion (soft locking): a converged column stays in
        X and keeps taking part in the Ritz step, but its W = T r is rounding noise and its P the difference of two nearly equal
        vectors, and this pencil needs several hundred block-Jacobi iterations during which the first mode sits at its rounding
        floor -- with those columns in the basis about one such solve in twenty broke down on the 23 x 17 test plate."""
        active = [j for j in range(b) if not norms[j, 0] <= self.rtol * abs(lam[j]) * norms[j, 1]]
        return list(range(b)) + [at + j for j in active] + ([b + j for j in active] if at > b else [])

    def geometric_stiffness_apply(self, V: torch.Tensor) -> torch.Tensor:
        """``K_G V`` for a block ``[m, n_u, 2]``, ``1 <= m <= 24`` (fp64, storage order), at the model's current ``u_free``.  For
        tests and measurements."""
        V = self._block(V, "V")
        self._refresh()
        out = torch.empty_like(V)
        self._geom_into(V, out, V.shape[0])
        return out

    def mass_apply(self, V):
        raise NotImplementedError("BucklingSolver: the pencil is (K_G, K); there is no mass operator (ModalSolver.mass_apply)")

    def solve(self) -> BucklingInfo:
        lam, modes, rnorm, it, converged = self._iterate()
        theta = lam[:self.n_modes].copy()
        neg = theta < 0.0
        factors = np.full(theta.shape, np.inf)
        factors[neg] = -1.0 / theta[neg]
        info = BucklingInfo(theta=torch.from_numpy(theta), load_factors=torch.from_numpy(factors), n_buckling=int(neg.sum()),
                            modes=modes, residual_norms=torch.from_numpy(rnorm), iterations=it, converged=converged)
        self._last = info
        return info


def linear_buckling(model, loss_fn, solve: bool = False, b_force=None, t_force=None, **kw) -> BucklingInfo:
    """One-shot ``BucklingSolver(model, loss_fn, **kw).solve()``.  ``solve=True`` first runs
    ``solve_displacement_(model, loss_fn, b_force=b_force, t_force=t_force, precond=...)`` -- which writes ``model.u_free``, as
    it always does -- so that the prestress is the static equilibrium under those forces (the loss's defaults when None);
    without it the two force arguments are not read."""
    solver = BucklingSolver(model, loss_fn, **kw)            # argument errors before anything is written
    if solve:
        from .solve import solve_displacement_
        solve_displacement_(model, loss_fn, b_force=b_force, t_force=t_force, precond=solver.precond)
    return solver.solve()
