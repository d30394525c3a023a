"""Free-vibration modes of a TRI3 or QUAD4 model: the lowest eigenpairs of ``K_ff phi = lambda M_ff phi`` by block LOBPCG.

``K_ff`` is the operator the frozen-mesh solver applies at the model's CURRENT coordinates (``FrozenMeshSolver.apply`` /
``Quad4FrozenMeshSolver.apply``), ``M_ff`` the consistent (or lumped) mass over the free ``u`` rows, applied matrix-free by
``hfem_mass_apply`` (csrc/modal.hip).  The block-vector work of the iteration -- Gram matrices, basis recombination,
residuals, the block-Jacobi preconditioner -- runs in the kernels of the same file; the Rayleigh-Ritz problem (at most 24 x 24)
is solved on the host in fp64 with numpy, which costs ONE host synchronisation per iteration (one device -> host read of the two
Gram matrices and the residual record, at most 2 x 24 x 24 + 16 doubles).  No reference counterpart: the reference has no mass
matrix.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import require_linear
from .post import node_adjacency

F64 = torch.float64
MAX_BLOCK = 8                        # kernels: block width m <= 8, a stacked basis [X P W] has at most 24 vectors
GRAM_PARTIALS = 73728                # HFEM_BLOCK_GRAM_PARTIALS
RESIDUAL_PARTIALS = 16384            # HFEM_BLOCK_RESIDUAL_PARTIALS
_G = 3 * MAX_BLOCK                   # rows of the largest Gram matrix


@dataclass
class ModalInfo:
    """Outcome of ``ModalSolver.solve()``.  ``eigenvalues`` [n_modes]: ascending lambda = omega^2 (fp64, CPU);
    ``frequencies`` = sqrt(lambda) / 2 pi; ``modes`` [n_modes, n_u, 2]: fp64 on the model's device, rows in the storage order of
    ``u_free``, M-orthonormal; ``residual_norms`` [n_modes]: ||K x_j - lambda_j M x_j||_2; ``iterations``: LOBPCG iterations
    done; ``converged``: every one of the ``n_modes`` pairs met ``||K x - lambda M x||_2 <= rtol lambda ||M x||_2``."""
    eigenvalues: torch.Tensor
    frequencies: torch.Tensor
    modes: torch.Tensor
    residual_norms: torch.Tensor
    iterations: int
    converged: bool


PIVOT_TOL = 1e-4    # smallest Cholesky pivot of the unit-diagonal mass Gram at which a column still counts as independent


def rayleigh_ritz(gk: np.ndarray, gm: np.ndarray, n_take: int, n_required: int = None, order=None):
    """The Ritz step of the iteration on the host: the lowest ``n_take`` pairs of the pencil ``(S^T K S, S^T M S)``.

    Both matrices are symmetrised and scaled by ``diag(S^T M S)^-1/2`` (the columns of S differ by many orders of magnitude: the
    residual directions shrink as the iteration converges).  The scaled mass Gram is Cholesky-factored column by column in
    ``order`` (default: as stored); a column whose pivot falls below ``PIVOT_TOL`` -- it depends on the columns factored before
    it to working precision: the Gram matrix squares the condition of the basis, a pivot p costs the Ritz vectors about
    eps / p^2 of their digits -- is left out of the basis, and so is one with a non-finite entry or a non-positive diagonal.
    The factor of the columns that stay, in that ONE order, reduces the pencil to the standard symmetric problem solved by
    ``numpy.linalg.eigh``: nothing is factored or thresholded a second time.

    Returns ``(lambda [n_take], C [ms, n_take], dropped)`` with ``C^T (S^T M S) C = I`` and zero rows in ``C`` for the
    ``dropped`` columns, or ``None`` when one of the first ``n_required`` columns of ``order`` (default: all of them) had to be
    dropped, when fewer than ``n_take`` columns stay, or when ``gk`` is not finite on them."""
    ms = gm.shape[0]
    order = list(range(ms)) if order is None else [int(i) for i in order]
    n_required = len(order) if n_required is None else n_required
    gk, gm = 0.5 * (gk + gk.T), 0.5 * (gm + gm.T)
    d = np.diag(gm)
    ok = np.isfinite(gm).all(axis=1) & np.isfinite(d) & (d > 0.0)
    s = np.where(ok, 1.0 / np.sqrt(np.where(ok, d, 1.0)), 0.0)
    g = gm * s[:, None] * s[None, :]
    keep, L = [], np.zeros((ms, ms))
    for pos, i in enumerate(order):
        k = len(keep)
        if ok[i]:
            y = np.linalg.solve(L[:k, :k], g[keep, i]) if k else np.zeros(0)    # row k of the factor: L[:k,:k] y = g[keep, i]
            p2 = g[i, i] - y @ y
            if p2 >= PIVOT_TOL * PIVOT_TOL:
                L[k, :k], L[k, k] = y, math.sqrt(p2)
                keep.append(i)
                continue
        if pos < n_required:
            return None
    k = len(keep)
    if k < n_take or not np.isfinite(gk[np.ix_(keep, keep)]).all():
        return None
    Li = np.linalg.inv(L[:k, :k])                            # <= 24 x 24, triangular
    sk = s[keep]
    A = Li @ (gk[np.ix_(keep, keep)] * sk[:, None] * sk[None, :]) @ Li.T
    w, Z = np.linalg.eigh(0.5 * (A + A.T))
    coef = np.zeros((ms, n_take))
    coef[keep] = sk[:, None] * (Li.T @ Z[:, :n_take])
    return w[:n_take].copy(), coef, ms - k


class ModalSolver:
    """Lowest ``n_modes`` free-vibration pairs of a TRI3 or QUAD4 mesh model with an ``EnergyLoss2D`` (block LOBPCG, Knyazev).

    ``density``: rho of the mass (unit thickness, as in K); ``mass``: ``"consistent"`` (TRI3 ``rho |det J| / 24 (1 + delta_ab)``,
    QUAD4 ``rho sum_q N_a N_b |det J_q|`` over the 2x2 Gauss points -- exact for any bilinear cell) or ``"lumped"`` (the row sum
    on the diagonal); ``precond``: ``"amg"`` (one V-cycle per column and iteration) or ``"block_jacobi"`` (the 2x2 diagonal
    blocks of K); ``block``: width of the iterated block, default ``min(8, n_modes + 2)``, ``1 <= n_modes <= block <= 8`` --
    the columns past ``n_modes`` are guard vectors; ``seed``: of the initial block (normal vectors drawn on the host in the
    CALLER's row order, so the result does not depend on ``reorder``).

    Mode j is converged when ``||K x_j - lambda_j M x_j||_2 <= rtol lambda_j ||M x_j||_2``; the solve stops when the first
    ``n_modes`` are, or after ``max_iter`` iterations.  Per iteration: the residual kernel; ``W = T R``; ``K W`` by ``block``
    calls of ``hfem_cg_apply`` and ``M W`` by one mass launch; the Gram matrices of ``S = [X P W]`` against ``K S`` and ``M S``;
    ONE device -> host read (the host synchronisation of the iteration: the Ritz problem is at most 24 x 24 and is solved with
    numpy); the new ``X, P, KX, KP, MX, MP`` as linear combinations of the held vectors (neither K nor M is applied again).
    ``P`` is absent in iteration 0; the mass Gram is Cholesky-factored in the order ``X``, ``W``, ``P``, and a ``W`` or ``P``
    column whose pivot falls below ``PIVOT_TOL`` is left out of that step (``rayleigh_ritz``) -- all of ``P`` left out is the
    classical restart -- and when ``X`` itself is dependent the solve stops with ``converged=False`` and the last good ``X``.
    ``restarts`` counts the steps of the last ``solve()`` that left columns out.  Convergence is read with the Gram matrices,
    so it is seen one iteration late: every solve pays one preconditioner, ``K`` and ``M`` application of the block past the
    iteration that converged.

    It owns a ``FrozenMeshSolver`` / ``Quad4FrozenMeshSolver`` for ``K p``, the block diagonal, the V-cycle and the refresh
    bookkeeping: ``solve()`` refreshes by the same state key when the coordinates moved.  ``model.u_free``, the coordinates and
    every ``.grad`` are left untouched.  fp32 models are solved in fp64 on their widened rows; results are fp64.

    THE NUMBERS ARE PHYSICAL ONLY WITH ``grad_convention="physical"`` (as the ZZ estimate): in the reference convention K is
    still the symmetric positive definite Hessian of the energy the model minimises, so the eigenproblem is well posed and is
    solved the same way, but its frequencies are not those of the elastic body.  K is the Hessian of the energy ``loss_fn``
    computes: a TRI3 loss with the default ``gauss_order=4`` carries the reference's extra factor 1/2 on the strain energy (its
    weights sum to 1/4), which halves every lambda; ``gauss_order=1`` (weights sum to 1/2) gives the plate's own.  Rigid-body
    modes are out of scope: the model needs Dirichlet rows."""

    _who = "ModalSolver"                 # the name in error messages (BucklingSolver iterates the same loop on another pencil)

    def __init__(self, model, loss_fn, n_modes: int = 6, density: float = 1.0, mass: str = "consistent", precond: str = "amg",
                 rtol: float = 1e-8, max_iter: int = 200, block=None, seed: int = 0):
        require_linear(loss_fn, self._who)
        npe = getattr(model, "nodes_per_element", 3)
        if npe not in (3, 4) or not hasattr(model, "_conn32"):
            raise NotImplementedError(f"{self._who}: TRI3 and QUAD4 mesh models")
        if mass not in ("consistent", "lumped"):
            raise ValueError("mass must be 'consistent' or 'lumped'")
        if precond not in ("amg", "block_jacobi"):
            raise ValueError("precond must be 'amg' or 'block_jacobi'")
        n_modes = int(n_modes)
        block = min(MAX_BLOCK, n_modes + 2) if block is None else int(block)
        if not 1 <= n_modes <= block <= MAX_BLOCK:
            raise ValueError(f"{self._who}: 1 <= n_modes <= block <= {MAX_BLOCK} (got n_modes={n_modes}, block={block})")
        if not float(density) > 0.0:
            raise ValueError("density must be > 0")
        if rtol <= 0 or int(max_iter) < 1:
            raise ValueError("rtol must be > 0 and max_iter >= 1")
        if int(model._idx_udir.shape[0]) == 0:
            raise ValueError(f"{self._who} needs Dirichlet rows: without them K_ff is singular (rigid-body modes are out of scope)")
        n_u = int(model.u_free.shape[0])
        if 2 * n_u < 3 * block:
            raise ValueError(f"{self._who}: the basis [X P W] of 3 x block = {3 * block} vectors needs at least as many free "
                             f"dofs (the model has {2 * n_u}); lower block or n_modes")
        cls = _frozen_class(npe)
        self.solver = cls(model, loss_fn, precond=precond)          # refuses a CPU model: there is no CPU fallback
        self.model, self.loss_fn, self.npe = model, loss_fn, npe
        self.n_modes, self.block, self.density, self.mass, self.precond = n_modes, block, float(density), mass, precond
        self.rtol, self.max_iter, self.seed = float(rtol), int(max_iter), int(seed)
        self.device = dev = self.solver.device
        self.n_u, self.len = n_u, 2 * n_u
        adj_ptr, adj = node_adjacency(model._conn32, model.Nnodes)
        self._adj_ptr, self._adj = adj_ptr.to(dev), adj.to(dev)
        self._row_node = model._idx_ufree.to(device=dev, dtype=torch.int32).contiguous()
        node_row = torch.full((model.Nnodes,), -1, dtype=torch.int32, device=dev)
        node_row[self._row_node.long()] = torch.arange(n_u, dtype=torch.int32, device=dev)
        self._node_row = node_row
        z = dict(dtype=F64, device=dev)
        self._gram_partials = torch.empty(GRAM_PARTIALS, **z)
        self._res_partials = torch.empty(RESIDUAL_PARTIALS, **z)
        self._rec = torch.zeros(2 * _G * _G + 2 * MAX_BLOCK, **z)         # {S^T K S, S^T M S, (|R_k|, |MX_k|) per column}
        self._coef = torch.zeros(_G * 2 * MAX_BLOCK + MAX_BLOCK, **z)     # {C [ms][mo], lambda [block]}
        self._pq = torch.empty((), **z)                                   # hfem_cg_apply's p^T q (not read)
        self._x64 = None
        self.restarts = 0
        self._key = None
        self._last = None

    # ---- operators on blocks [m, n_u, 2] (fp64, storage order)
    def _refresh(self):
        if self._key is None or self._key != self.solver._state_key():
            self.solver.refresh()
            with torch.no_grad():
                self._x64 = self.model.coords.detach().to(F64).contiguous()
            self._key = self.solver._state_key()

    def _block(self, V, name):
        V = _lib.require_gpu_tensor(V.detach(), name, F64)
        if V.dim() != 3 or V.shape[1:] != (self.n_u, 2) or not 1 <= V.shape[0] <= _G:
            raise ValueError(f"{name}: a block [m, {self.n_u}, 2] with 1 <= m <= {_G}")
        return V

    def _mass_into(self, V, out, m):
        """out[:m] = M V[:m] (any m: the entry point takes at most 8 columns a call)."""
        md = self.model
        for k in range(0, m, MAX_BLOCK):
            mk = min(MAX_BLOCK, m - k)
            check(_lib.lib().hfem_mass_apply(_lib.dev_index(self.device), self.npe, ptr(self._x64), ptr(md._conn32), md.Nelems,
                                             md.Nnodes, ptr(self._adj_ptr), ptr(self._adj), ptr(self._row_node),
                                             ptr(self._node_row), self.n_u, self.density, 1 if self.mass == "lumped" else 0,
                                             ptr(V[k]), mk, ptr(out[k]), stream_ptr(self.device)), "hfem_mass_apply")

    def _stiffness_into(self, V, out, m):
        h, s = self.solver._h, stream_ptr(self.device)
        for k in range(m):
            check(_lib.lib().hfem_cg_apply(h, ptr(V[k]), ptr(out[k]), ptr(self._pq), s), "hfem_cg_apply")

    # the two operators of the pencil A x = lambda B x as the loop of _iterate() reaches them: here (K, M)
    def _a_into(self, V, out, m):
        self._stiffness_into(V, out, m)

    def _b_into(self, V, out, m):
        self._mass_into(V, out, m)

    def mass_apply(self, V: torch.Tensor) -> torch.Tensor:
        """``M_ff V`` for a block ``[m, n_u, 2]`` (fp64, storage order).  For tests and measurements."""
        V = self._block(V, "V")
        self._refresh()
        out = torch.empty_like(V)
        self._mass_into(V, out, V.shape[0])
        return out

    def stiffness_apply(self, V: torch.Tensor) -> torch.Tensor:
        """``K_ff V`` for a block ``[m, n_u, 2]`` (fp64, storage order).  For tests and measurements."""
        V = self._block(V, "V")
        self._refresh()
        out = torch.empty_like(V)
        self._stiffness_into(V, out, V.shape[0])
        return out

    def _precondition_into(self, R, W, m):
        if self.precond == "amg":
            a, s = self.solver._amg._h, stream_ptr(self.device)
            for k in range(m):
                check(_lib.lib().hfem_amg_vcycle(a, ptr(R[k]), ptr(W[k]), s), "hfem_amg_vcycle")
        else:
            check(_lib.lib().hfem_block_jacobi_apply(_lib.dev_index(self.device), ptr(self.solver.diag), ptr(R), m, self.len, ptr(W),
                                                     stream_ptr(self.device)), "hfem_block_jacobi_apply")

    def _residual_into(self, KS, MS, R, m):
        """R[k] = KX[k] - lambda_k MX[k] for the leading m vectors of the held sets, the two norms per column into the record."""
        check(_lib.lib().hfem_block_residual(_lib.dev_index(self.device), ptr(KS), ptr(MS), ptr(self._coef[_G * 2 * MAX_BLOCK:]), m,
                                             self.len, ptr(R), ptr(self._res_partials), ptr(self._rec[2 * _G * _G:]),
                                             stream_ptr(self.device)), "hfem_block_residual")

    def _grams(self, S, KS, MS, ms):
        """S^T K S and S^T M S into the device record (no host read)."""
        d, s = _lib.dev_index(self.device), stream_ptr(self.device)
        gk, gm = self._rec[:_G * _G], self._rec[_G * _G:2 * _G * _G]
        check(_lib.lib().hfem_block_gram(d, ptr(S), ms, ptr(KS), ms, self.len, ptr(self._gram_partials), ptr(gk), s), "hfem_block_gram")
        check(_lib.lib().hfem_block_gram(d, ptr(S), ms, ptr(MS), ms, self.len, ptr(self._gram_partials), ptr(gm), s), "hfem_block_gram")

    def _read(self, ms):
        """The one device -> host read of an iteration: (S^T K S, S^T M S, residual record)."""
        rec = self._rec.cpu().numpy()
        gk = rec[:ms * ms].reshape(ms, ms)
        gm = rec[_G * _G:_G * _G + ms * ms].reshape(ms, ms)
        return gk, gm, rec[2 * _G * _G:].reshape(MAX_BLOCK, 2)

    def _combine(self, coef, lam, src, dst, ms, mo):
        """dst[i][:mo] = sum_k coef[k, :] src[i][k] for the three held sets (S, KS, MS); lambda goes up in the same copy."""
        host = np.zeros(self._coef.numel())
        host[:ms * mo] = np.ascontiguousarray(coef).reshape(-1)
        host[_G * 2 * MAX_BLOCK:_G * 2 * MAX_BLOCK + lam.shape[0]] = lam
        self._coef.copy_(torch.from_numpy(host))
        d, s = _lib.dev_index(self.device), stream_ptr(self.device)
        for a, b in zip(src, dst):
            check(_lib.lib().hfem_block_combine(d, ptr(a), ms, ptr(self._coef), mo, self.len, ptr(b), s), "hfem_block_combine")

    def _initial_block(self):
        rng = np.random.default_rng(self.seed)
        v = torch.from_numpy(rng.standard_normal((self.n_u, self.block, 2)))      # rows in the caller's order
        return self.model.from_caller_order(v, "u").transpose(0, 1).contiguous().to(self.device)

    def _ritz_order(self, b, at, ms, norms, lam):
        """The basis columns of a Ritz step in the order their Gram matrix is factored: X, W, P, all of them."""
        return list(range(b)) + list(range(at, ms)) + list(range(b, at))

    def _iterate(self):
        """The LOBPCG loop on the pencil (``_a_into``, ``_b_into``): ``(lambda [block], modes [n_modes, n_u, 2], residual norms
        [n_modes], iterations, converged)``."""
        self._refresh()
        b, nm, n = self.block, self.n_modes, self.n_u
        self.restarts = 0                                     # Ritz steps of this solve that had to drop basis columns
        with torch.no_grad():
            z = dict(dtype=F64, device=self.device)
            # two sets of [X P W] x {S, KS, MS}: the combine kernel writes the new X and P into the other set
            cur = [torch.zeros((3 * b, n, 2), **z) for _ in range(3)]
            nxt = [torch.zeros((3 * b, n, 2), **z) for _ in range(3)]
            S, KS, MS = cur
            S[:b].copy_(self._initial_block())
            self._a_into(S, KS, b)
            self._b_into(S, MS, b)
            self._grams(S, KS, MS, b)
            gk, gm, _ = self._read(b)
            rr = rayleigh_ritz(gk, gm, b)
            if rr is None:
                raise RuntimeError(f"{self._who}: the initial block is not linearly independent in the inner product of the pencil")
            lam, coef, _ = rr
            self._combine(coef, lam, cur, nxt, b, b)
            cur, nxt = nxt, cur
            have_p, it, converged = False, 0, False
            rnorm = np.full(nm, np.inf)
            while True:
                S, KS, MS = cur
                # W goes behind the held vectors: slot 1 while P is absent, slot 2 otherwise
                at = 2 * b if have_p else b
                ms = at + b
                W = S[at:ms]
                if self.precond == "amg":                     # the V-cycle is out of place: R sits in the KW slot for a moment
                    self._residual_into(KS, MS, KS[at:ms], b)
                    self._precondition_into(KS[at:ms], W, b)
                else:
                    self._residual_into(KS, MS, W, b)
                    self._precondition_into(W, W, b)
                self._a_into(W, KS[at:ms], b)
                self._b_into(W, MS[at:ms], b)
                self._grams(S, KS, MS, ms)
                gk, gm, norms = self._read(ms)               # the host synchronisation of the iteration
                rnorm = norms[:nm, 0].copy()
                converged = bool((norms[:nm, 0] <= self.rtol * np.abs(lam[:nm]) * norms[:nm, 1]).all())
                if converged or it >= self.max_iter:
                    break
                # the mass Gram is factored in the order X, W, P: a W or P column that depends on the ones before it is left
                # out of this step (all of P left out = the classical restart).  X itself dependent: stop with the last good X.
                order = self._ritz_order(b, at, ms, norms, lam)
                rr = rayleigh_ritz(gk, gm, b, n_required=b, order=order)
                if rr is None:
                    break
                lam, cx, dropped = rr
                self.restarts += int(dropped > ms - len(order))
                cp = cx.copy()
                cp[:b] = 0.0                                  # P = the part of the new X that is not in the old X
                self._combine(np.concatenate([cx, cp], axis=1), lam, cur, nxt, ms, 2 * b)
                cur, nxt = nxt, cur
                have_p = True
                it += 1
            modes = cur[0][:nm].clone()
        return lam, modes, rnorm, it, converged

    def solve(self) -> ModalInfo:
        lam, modes, rnorm, it, converged = self._iterate()
        nm = self.n_modes
        lam_t = torch.from_numpy(lam[:nm].copy())
        info = ModalInfo(eigenvalues=lam_t, frequencies=torch.sqrt(lam_t.clamp_min(0.0)) / (2.0 * math.pi), modes=modes,
                         residual_norms=torch.from_numpy(rnorm), iterations=it, converged=converged)
        self._last = info
        return info

    def modes_in_caller_order(self, modes=None) -> torch.Tensor:
        """``modes`` (default: those of the last ``solve()``) ``[n_modes, n_u, 2]`` with rows in the caller's numbering
        (``model.to_caller_order(..., "u")`` per mode)."""
        if modes is None:
            if self._last is None:
                raise RuntimeError("modes_in_caller_order(): call solve() first")
            modes = self._last.modes
        return self.model.to_caller_order(modes.transpose(0, 1).contiguous(), "u").transpose(0, 1).contiguous()


def _frozen_class(npe):
    from .solve import FrozenMeshSolver, Quad4FrozenMeshSolver
    return Quad4FrozenMeshSolver if npe == 4 else FrozenMeshSolver


def vibration_modes(model, loss_fn, **kw) -> ModalInfo:
    """One-shot ``ModalSolver(model, loss_fn, **kw).solve()``."""
    return ModalSolver(model, loss_fn, **kw).solve()
