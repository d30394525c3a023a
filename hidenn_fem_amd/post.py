"""Post-processing on the device: the compute cores of the reference's plotting helpers
(``/root/reference/src/plots.py``), without matplotlib and without per-element Python loops.

* ``von_mises(model, E, nu)``  -- ``plots.plot_von_mises`` (plots.py:177-198) up to the array it colours the
  triangles with: centroid ``grad_u`` -> strain -> plane-stress stress -> von Mises, one fused kernel.
* ``compute_du_dx_per_element(model)`` -- plots.py:5-27 (one ``autograd.grad`` call per element in a Python
  loop there): the per-element slope of the 1D piecewise-linear field, one kernel.

No reference counterpart: ``StressRecovery`` / ``recover_stress`` / ``zz_error`` -- the nodal (smoothed) stress
by lumped L2 projection and the Zienkiewicz-Zhu energy-norm error estimate built on it, TRI3 and QUAD4 models
(csrc/recover.hip); ``von_mises`` of a QUAD4 model is taken at the cell centre.
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
