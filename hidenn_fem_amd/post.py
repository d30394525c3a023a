"""Post-processing on the device: the compute cores of the reference's plotting helpers
(``/root/reference/src/plots.py``), without matplotlib and without per-element Python loops.

* ``von_mises(model, E, nu)``  -- ``plots.plot_von_mises`` (plots.py:177-198) up to the array it colours the
  triangles with: centroid ``grad_u`` -> strain -> plane-stress stress -> von Mises, one fused kernel.
* ``compute_du_dx_per_element(model)`` -- plots.py:5-27 (one ``autograd.grad`` call per element in a Python
  loop there): the per-element slope of the 1D piecewise-linear field, one kernel.

No reference counterpart: ``StressRecovery`` / ``recover_stress`` / ``zz_error`` -- the nodal (smoothed) stress
by lumped L2 projection and the Zienkiewicz-Zhu energy-norm error estimate built on it, TRI3 and QUAD4 models
(csrc/recover.hip); ``von_mises`` of a QUAD4 model is taken at the cell centre.  Their finite-strain twins:
``HyperStressRecovery`` / ``recover_cauchy_stress`` / ``hyper_zz_error`` -- the recovered Cauchy stress of a Neo-Hookean
model and a ZZ indicator on it, the same kernels with another stress law.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, require_gpu_tensor
from .loss import HFEM_FLAG_PHYSICAL_GRAD

F64 = torch.float64


def von_mises(model, E: float = 10e9, nu: float = 0.3, return_grad_u: bool = False):
    """Per-element von Mises stress [Ne] (and optionally the centroid ``grad_u`` [Ne,2,2]) of a triangular
    model; dtype of ``model.coords``.  QUAD4 models: the same chain at the cell centre (xi = eta = 0)."""
    if getattr(model, "nodes_per_element", 3) == 4:
        return _quad4_von_mises(model, E, nu, return_grad_u)
    with torch.no_grad():
        X, U = model.coords.detach(), model.u_full.detach()
        require_gpu_tensor(X.contiguous(), "model.coords", dtype=None)
        dt = X.dtype
        X64, U64 = X.to(F64).contiguous(), U.to(F64).contiguous()
        ne = model.Nelems
        vm = torch.empty(ne, dtype=F64, device=X.device)
        gu = torch.empty(ne, 2, 2, dtype=F64, device=X.device) if return_grad_u else None
        check(_lib.lib().hfem_tri3_von_mises(_lib.dev_index(X.device), ptr(X64), ptr(U64), ptr(model._conn32), ne, float(E),
                                             float(nu), ptr(vm), ptr(gu), stream_ptr(X.device)), "hfem_tri3_von_mises")
        vm = vm.to(dt)
        return (vm, gu.to(dt)) if return_grad_u else vm


def _quad4_von_mises(model, E, nu, return_grad_u):
    with torch.no_grad():
        X, U = model.coords.detach(), model.u_full.detach()
        require_gpu_tensor(X.contiguous(), "model.coords", dtype=None)
        dt = X.dtype
        X64, U64 = X.to(F64).contiguous(), U.to(F64).contiguous()
        ne = model.Nelems
        vm = torch.empty(ne, dtype=F64, device=X.device)
        gu = torch.empty(ne, 2, 2, dtype=F64, device=X.device) if return_grad_u else None
        check(_lib.lib().hfem_quad4_von_mises(_lib.dev_index(X.device), ptr(X64), ptr(U64), ptr(model._conn32), ne, float(E),
                                              float(nu), ptr(vm), ptr(gu), stream_ptr(X.device)), "hfem_quad4_von_mises")
        vm = vm.to(dt)
        return (vm, gu.to(dt)) if return_grad_u else vm


def compute_du_dx_per_element(model) -> torch.Tensor:
    """du/dx on every element of a 1D model ([Ne] for scalar u, [Ne, dim_u] otherwise), returned on the CPU
    like the reference's helper."""
    with torch.no_grad():
        grid, u = model.grid.detach(), model.u_full.detach()
        require_gpu_tensor(grid.contiguous(), "model.grid", dtype=None)
        g64 = grid.to(F64).contiguous()
        u64 = u.to(F64).reshape(grid.shape[0], -1).contiguous()
        dim_u = u64.shape[1]
        out = torch.empty(grid.shape[0] - 1, dim_u, dtype=F64, device=grid.device)
        check(_lib.lib().hfem_line2_slopes(_lib.dev_index(grid.device), ptr(g64), ptr(u64), grid.shape[0], dim_u, ptr(out),
                                           stream_ptr(grid.device)), "hfem_line2_slopes")
        out = out.to(grid.dtype).cpu()
        return out[:, 0] if dim_u == 1 else out


# ---------------------------------------------------------------- nodal stress recovery, ZZ error estimate
ADJ_MAX_ELEMS = 1 << 29      # adjacency entries are ``e << 2 | c`` in int32


def node_adjacency(conn, n_nodes: int):
    """Node -> (element, corner) adjacency of a connectivity ``[Ne, 3 or 4]`` as CSR: ``(adj_ptr [n_nodes + 1], adj [npe * Ne])``,
    int32 CPU tensors, entries ``e << 2 | c``; at every node they ascend in the element id (stable sort of the flattened
    connectivity) -- the fixed order the recovery kernel adds in.  ``ValueError`` for ``Ne >= 2**29`` (the packing)."""
    ne, npe = int(conn.shape[0]), int(conn.shape[1])
    if ne >= ADJ_MAX_ELEMS:
        raise ValueError(f"node_adjacency: {ne} elements; entries are packed e << 2 | c in int32, so Ne < 2**29")
    if npe not in (3, 4):
        raise ValueError("node_adjacency: connectivity [Ne, 3] or [Ne, 4]")
    flat = (conn.detach().cpu().numpy() if isinstance(conn, torch.Tensor) else np.asarray(conn)).reshape(-1).astype(np.int64)
    if flat.size and (flat.min() < 0 or flat.max() >= n_nodes):
        raise ValueError("node_adjacency: node id out of range")
    order = np.argsort(flat, kind="stable")                 # flattened position = npe * e + c: ascending e at equal node
    packed = ((order // npe) << 2 | (order % npe)).astype(np.int32)
    adj_ptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=n_nodes), out=adj_ptr[1:])
    return torch.from_numpy(adj_ptr.astype(np.int32)), torch.from_numpy(packed)


@dataclass
class ZZError:
    """Result of ``StressRecovery.error()``.  ``eta2`` [Ne]: element indicators eta_e^2; ``energy_norm2``: ||u_h||^2 = twice
    the strain energy; ``eta`` = sqrt(sum eta_e^2); ``relative`` = sqrt(eta^2 / (||u_h||^2 + eta^2)); ``nodal_stress`` [Nn, 3]
    the recovered field the indicators were built on.  The three scalars are Python floats (one device read)."""
    eta2: torch.Tensor
    energy_norm2: float
    eta: float
    relative: float
    nodal_stress: torch.Tensor


class StressRecovery:
    """Recovered nodal stress and ZZ error estimate of a TRI3 or QUAD4 model.

    sigma = C (eps_xx, eps_yy, gamma_xy) with C and the gradient convention of ``loss_fn`` (``EnergyLoss2D``); points: the
    centroid with weight |det J| / 2 (TRI3), the 2x2 Gauss points with |det J_q| (QUAD4).  ``nodal_stress()``: lumped L2
    projection sigma*_n = sum w_q N_n(q) sigma_h(q) / sum w_q N_n(q) over the elements at n; ``error()``: eta_e^2 =
    int_e (sigma* - sigma_h).S.(sigma* - sigma_h), S = C^-1, and ||u_h||^2 = int sigma_h.S.sigma_h.

    eta ESTIMATES THE DISCRETISATION ERROR ONLY WITH ``grad_convention="physical"``: in the reference convention sigma_h is
    not the stress of u_h (a linear displacement field does not give eta = 0 there), the quantities are merely computed
    the same way.

    The adjacency is built and uploaded once (the connectivity never changes); ``model.coords`` / ``model.u_full`` are read
    on every call, so one object stays valid across r-adaptive steps.  fp32 models are widened on the way in and get fp32
    results back."""

    def __init__(self, model, loss_fn):
        from .loss import require_linear
        require_linear(loss_fn, "StressRecovery")
        npe = getattr(model, "nodes_per_element", 3)
        if npe not in (3, 4) or not hasattr(model, "_conn32"):
            raise NotImplementedError("StressRecovery: TRI3 and QUAD4 mesh models")
        self.model, self.loss_fn, self.npe = model, loss_fn, npe
        dev = model.node_coords_free.device
        if dev.type != "cuda":
            raise RuntimeError(f"hidenn_fem_amd: model is on {dev}; the recovery kernels need a ROCm device. "
                               "There is no CPU fallback -- call model.to('cuda').")
        self.device = dev
        adj_ptr, adj = node_adjacency(model._conn32, model.Nnodes)
        self._adj_ptr, self._adj = adj_ptr.to(dev), adj.to(dev)
        self._partials = torch.empty(2 * max((model.Nelems + 255) // 256, 1), dtype=F64, device=dev)
        self._mat = (C.c_double * 4)(*loss_fn._mat)
        L = _lib.lib()
        self._recover = L.hfem_quad4_stress_recover if npe == 4 else L.hfem_tri3_stress_recover
        self._zz = L.hfem_quad4_zz_error if npe == 4 else L.hfem_tri3_zz_error
        self._name = "quad4" if npe == 4 else "tri3"

    def _inputs(self):
        m = self.model
        X, U = m.coords.detach(), m.u_full.detach()
        require_gpu_tensor(X.contiguous(), "model.coords", dtype=None)
        return X.dtype, X.to(F64).contiguous(), U.to(F64).contiguous(), self.loss_fn._mode_flags(m) & HFEM_FLAG_PHYSICAL_GRAD

    def _nodal(self, X64, U64, flags, area):
        m = self.model
        sig = torch.empty(m.Nnodes, 3, dtype=F64, device=self.device)
        check(self._recover(_lib.dev_index(self.device), ptr(X64), ptr(U64), ptr(m._conn32), m.Nelems, m.Nnodes,
                            ptr(self._adj_ptr), ptr(self._adj), self._mat, flags, ptr(sig), ptr(area),
                            stream_ptr(self.device)), f"hfem_{self._name}_stress_recover")
        return sig

    def nodal_stress(self, return_area: bool = False):
        """Recovered stress ``[Nnodes, 3]`` = (sxx, syy, sxy) by node id (and the lumped nodal areas ``[Nnodes]``)."""
        with torch.no_grad():
            dt, X64, U64, flags = self._inputs()
            area = torch.empty(self.model.Nnodes, dtype=F64, device=self.device) if return_area else None
            sig = self._nodal(X64, U64, flags, area).to(dt)
            return (sig, area.to(dt)) if return_area else sig

    def nodal_von_mises(self):
        """Plane-stress von Mises of the recovered stress, ``[Nnodes]``."""
        s = self.nodal_stress()
        return torch.sqrt(s[:, 0] ** 2 - s[:, 0] * s[:, 1] + s[:, 1] ** 2 + 3.0 * s[:, 2] ** 2)

    def error(self) -> ZZError:
        with torch.no_grad():
            m = self.model
            dt, X64, U64, flags = self._inputs()
            sig = self._nodal(X64, U64, flags, None)
            eta2 = torch.empty(m.Nelems, dtype=F64, device=self.device)
            totals = torch.zeros(2, dtype=F64, device=self.device)
            check(self._zz(_lib.dev_index(self.device), ptr(X64), ptr(U64), ptr(m._conn32), m.Nelems, ptr(sig), self._mat,
                           flags, ptr(eta2), None, ptr(self._partials), ptr(totals), stream_ptr(self.device)),
                  f"hfem_{self._name}_zz_error")
            e2, n2 = totals.tolist()
            rel = (e2 / (n2 + e2)) ** 0.5 if n2 + e2 > 0.0 else 0.0
            return ZZError(eta2=eta2.to(dt), energy_norm2=n2, eta=e2 ** 0.5, relative=rel, nodal_stress=sig.to(dt))


def recover_stress(model, loss_fn) -> torch.Tensor:
    """One-shot ``StressRecovery(model, loss_fn).nodal_stress()``."""
    return StressRecovery(model, loss_fn).nodal_stress()


def zz_error(model, loss_fn) -> ZZError:
    """One-shot ``StressRecovery(model, loss_fn).error()``."""
    return StressRecovery(model, loss_fn).error()


# ---------------------------------------------------------------- Cauchy stress recovery, ZZ indicator at finite strain
@dataclass
class HyperZZError(ZZError):
    """Result of ``HyperStressRecovery.error()``: ``ZZError``'s fields (``nodal_stress`` is the recovered CAUCHY stress) plus
    ``min_J`` = min det F over all points and ``inverted`` = the number of inverted elements.  With ``inverted > 0`` those
    elements' ``eta2`` is ``+inf``, ``eta`` is ``inf`` and ``relative`` is 1.0.  The four scalars come from one device read."""
    min_J: float = float("nan")
    inverted: int = 0


class HyperStressRecovery:
    """Recovered nodal Cauchy stress and a ZZ error indicator of a finite-strain model: a ``NeoHookeanLoss2D`` on a TRI3 model
    or a ``Quad4NeoHookeanLoss2D`` on a QUAD4 model (the same kernels as ``StressRecovery`` with another stress law,
    csrc/recover.hip).

    ``(lambda, mu) = loss_fn.lame``; per point ``H = G J^-1`` (always the physical gradient), ``F = I + H``,
    ``j = tr H + det H = det F - 1`` and ``sigma_h = (mu (H + H^T + H H^T) + lambda log1p(j) I) / (1 + j)`` -- the Cauchy stress
    ``P F^T / det F`` of the energy the model was solved with, in a cancellation-free form.  Points and weights are
    ``StressRecovery``'s, taken on the reference configuration, and so is the lumped L2 projection; ``return_J`` gives the
    same projection of ``det F``.  ``error()``: ``eta_e^2 = int_e (sigma* - sigma_h).S.(sigma* - sigma_h) dX`` and
    ``||sigma_h||^2 = int sigma_h.S.sigma_h dX`` with ``S = C0^-1``, ``C0`` the linearisation of the material at ``F = I``
    (``c11 = c22 = lambda + 2 mu, c12 = lambda, c33 = mu``; ``plane="stress"``: ``EnergyLoss2D.C`` entry for entry).

    * IT IS AN INDICATOR, NOT AN ESTIMATE, AWAY FROM SMALL STRAIN: ``S`` is the compliance at the undeformed state, so ``eta`` is
      no bound of an error in an energy norm of the deformed body; it says where the stress jumps between elements.
    * It reduces to the linear ZZ estimate of ``EnergyLoss2D(grad_convention="physical")`` as ``u -> 0``.
    * It is exactly zero for a homogeneous deformation, and unchanged by a superposed rigid rotation because ``S`` is isotropic
      (the recovered stress turns with the body: ``sigma* -> Q sigma* Q^T``).

    Inverted elements (``det F <= 0`` or NaN at a point; a QUAD4 cell when any of its four points is): weight 0 in the
    projection, ``eta_e^2 = +inf``, nothing added to ``||sigma_h||^2``; a node all of whose elements are inverted gets zeros and
    lumped area 0; ``relative`` is 1.0.  No NaN arises from finite inputs.

    The adjacency is built and uploaded once; ``model.coords`` / ``model.u_full`` are read on every call, so one object stays
    valid across r-adaptive steps and load increments.  fp32 models are widened on the way in and get fp32 results back."""

    def __init__(self, model, loss_fn):
        from .loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
        npe = getattr(model, "nodes_per_element", 3)
        if not isinstance(loss_fn, NeoHookeanLoss2D):
            raise NotImplementedError("HyperStressRecovery: a NeoHookeanLoss2D (TRI3) or Quad4NeoHookeanLoss2D (QUAD4); the "
                                      "small-strain stress of an EnergyLoss2D is hidenn_fem_amd.post.StressRecovery")
        if npe not in (3, 4) or not hasattr(model, "_conn32"):
            raise NotImplementedError("HyperStressRecovery: TRI3 and QUAD4 mesh models")
        if isinstance(loss_fn, Quad4NeoHookeanLoss2D) != (npe == 4):
            raise NotImplementedError("HyperStressRecovery: NeoHookeanLoss2D goes with a TRI3 model, Quad4NeoHookeanLoss2D with "
                                      f"a QUAD4 model (got {type(loss_fn).__name__} and {npe} nodes per element)")
        self.model, self.loss_fn, self.npe = model, loss_fn, npe
        dev = model.node_coords_free.device
        if dev.type != "cuda":
            raise RuntimeError(f"hidenn_fem_amd: model is on {dev}; the recovery kernels need a ROCm device. "
                               "There is no CPU fallback -- call model.to('cuda').")
        self.device = dev
        adj_ptr, adj = node_adjacency(model._conn32, model.Nnodes)
        self._adj_ptr, self._adj = adj_ptr.to(dev), adj.to(dev)
        self._partials = torch.empty(4 * max((model.Nelems + 255) // 256, 1), dtype=F64, device=dev)
        self._lame = (C.c_double * 2)(*loss_fn.lame)
        L = _lib.lib()
        self._recover = L.hfem_quad4_hyper_stress_recover if npe == 4 else L.hfem_tri3_hyper_stress_recover
        self._zz = L.hfem_quad4_hyper_zz_error if npe == 4 else L.hfem_tri3_hyper_zz_error
        self._name = "quad4" if npe == 4 else "tri3"

    def _inputs(self):
        m = self.model
        X, U = m.coords.detach(), m.u_full.detach()
        require_gpu_tensor(X.contiguous(), "model.coords", dtype=None)
        return X.dtype, X.to(F64).contiguous(), U.to(F64).contiguous()

    def _nodal(self, X64, U64, J, area):
        m = self.model
        sig = torch.empty(m.Nnodes, 3, dtype=F64, device=self.device)
        check(self._recover(_lib.dev_index(self.device), ptr(X64), ptr(U64), ptr(m._conn32), m.Nelems, m.Nnodes,
                            ptr(self._adj_ptr), ptr(self._adj), self._lame, ptr(sig), ptr(J), ptr(area),
                            stream_ptr(self.device)), f"hfem_{self._name}_hyper_stress_recover")
        return sig

    def nodal_stress(self, return_area: bool = False, return_J: bool = False):
        """Recovered Cauchy stress ``[Nnodes, 3]`` = (sxx, syy, sxy) by node id; then, as asked, the lumped nodal areas
        ``[Nnodes]`` (reference configuration) and the recovered ``det F`` ``[Nnodes]``, in that order."""
        with torch.no_grad():
            dt, X64, U64 = self._inputs()
            nn = self.model.Nnodes
            area = torch.empty(nn, dtype=F64, device=self.device) if return_area else None
            J = torch.empty(nn, dtype=F64, device=self.device) if return_J else None
            out = (self._nodal(X64, U64, J, area).to(dt),)
            out += (area.to(dt),) if return_area else ()
            out += (J.to(dt),) if return_J else ()
            return out if len(out) > 1 else out[0]

    def nodal_von_mises(self):
        """Plane-stress von Mises of the recovered Cauchy stress, ``[Nnodes]``."""
        s = self.nodal_stress()
        return torch.sqrt(s[:, 0] ** 2 - s[:, 0] * s[:, 1] + s[:, 1] ** 2 + 3.0 * s[:, 2] ** 2)

    def error(self) -> HyperZZError:
        with torch.no_grad():
            m = self.model
            dt, X64, U64 = self._inputs()
            sig = self._nodal(X64, U64, None, None)
            eta2 = torch.empty(m.Nelems, dtype=F64, device=self.device)
            totals = torch.zeros(4, dtype=F64, device=self.device)
            check(self._zz(_lib.dev_index(self.device), ptr(X64), ptr(U64), ptr(m._conn32), m.Nelems, ptr(sig), self._lame,
                           ptr(eta2), None, ptr(self._partials), ptr(totals), stream_ptr(self.device)),
                  f"hfem_{self._name}_hyper_zz_error")
            e2, n2, min_j, count = totals.tolist()
            count = int(count)
            rel = 1.0 if count > 0 else ((e2 / (n2 + e2)) ** 0.5 if n2 + e2 > 0.0 else 0.0)
            return HyperZZError(eta2=eta2.to(dt), energy_norm2=n2, eta=e2 ** 0.5, relative=rel, nodal_stress=sig.to(dt),
                                min_J=min_j, inverted=count)


def recover_cauchy_stress(model, loss_fn) -> torch.Tensor:
    """One-shot ``HyperStressRecovery(model, loss_fn).nodal_stress()``."""
    return HyperStressRecovery(model, loss_fn).nodal_stress()


def hyper_zz_error(model, loss_fn) -> HyperZZError:
    """One-shot ``HyperStressRecovery(model, loss_fn).error()``."""
    return HyperStressRecovery(model, loss_fn).error()
