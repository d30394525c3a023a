"""CPU-torch fp64 statement of the Neo-Hookean tangent and of the inexact Newton solve on it, shared by the tests
(a plain helper module, not a conftest).  It imports ``hyper_reference`` and nothing from the library's compute paths.

Per element, in ``hyper_reference``'s notation (H, F = I + H, L = log1p(j), T = F^-T, A = |det Jg| W), the directional
derivative of the first Piola-Kirchhoff stress in the direction dH = dG Jg^-1, dG = [p0 - p2, p1 - p2]:

    dP = mu dH + (mu - lambda L) T dH^T T + lambda (T : dH) T
    q  = A dP Jg^-T          column a -> node a (a = 0, 1), minus the column sum -> node 2

Dead loads do not enter.  An element with j <= -1 contributes a zero block.

The driver is the algorithm of ``hidenn_fem_amd.newton.NewtonKrylovSolver`` on dense matrices: block-Jacobi PCG truncated on
p^T K p <= 0 (the direction reached so far; at CG iteration 0 the preconditioned steepest descent -M g), the forcing term of
Eisenstat-Walker choice 2, and backtracking on  Pi(u + t d) <= Pi(u) + armijo t g.d + 4 eps |Pi(u)|.
"""
from dataclasses import dataclass, field as _field

import torch

import hyper_reference as H

F64 = torch.float64
EPS = 2.2e-16


# ---------------------------------------------------------------- the tangent
def element_tangent(coords, u, conn, lam, mu, W):
    """-> Ke [Ne, 6, 6] over the dofs (node k, component c) -> 2 k + c; zero for an inverted element."""
    X, U, Jg, G = H._parts(coords, u, conn)
    ne = conn.shape[0]
    det = Jg[:, 0, 0] * Jg[:, 1, 1] - Jg[:, 0, 1] * Jg[:, 1, 0]
    Jinv = torch.stack([torch.stack([Jg[:, 1, 1], -Jg[:, 0, 1]], 1), torch.stack([-Jg[:, 1, 0], Jg[:, 0, 0]], 1)], 1) / det[:, None, None]
    Hm = G @ Jinv
    j = Hm[:, 0, 0] + Hm[:, 1, 1] + (Hm[:, 0, 0] * Hm[:, 1, 1] - Hm[:, 0, 1] * Hm[:, 1, 0])
    inverted = ~(j > -1.0)
    js = torch.where(inverted, torch.zeros_like(j), j)
    L = torch.log1p(js)
    F = torch.eye(2, dtype=F64).expand(ne, 2, 2) + Hm
    T = torch.stack([torch.stack([F[:, 1, 1], -F[:, 1, 0]], 1), torch.stack([-F[:, 0, 1], F[:, 0, 0]], 1)], 1) / (1.0 + js)[:, None, None]
    A = det.abs() * W * (~inverted).to(F64)
    c = mu - lam * L
    Ke = torch.zeros(ne, 6, 6, dtype=F64)
    for l in range(3):
        for comp in range(2):
            dG = torch.zeros(ne, 2, 2, dtype=F64)
            if l < 2:
                dG[:, comp, l] = 1.0
            else:
                dG[:, comp, :] = -1.0
            dH = dG @ Jinv
            tdh = (T * dH).sum(dim=(1, 2))
            dP = mu * dH + c[:, None, None] * (T @ dH.transpose(1, 2) @ T) + (lam * tdh)[:, None, None] * T
            Q = A[:, None, None] * (dP @ Jinv.transpose(1, 2))
            q = torch.stack([Q[:, :, 0], Q[:, :, 1], -(Q[:, :, 0] + Q[:, :, 1])], dim=1)      # [Ne, 3, 2]
            Ke[:, :, 2 * l + comp] = q.reshape(ne, 6)
    return Ke


def dense_tangent(coords, u, conn, lam, mu, W, skip=None):
    """K_T [2 Nn, 2 Nn] (dof 2 n + c).  ``skip``: a bool mask [Ne] of elements left out."""
    Ke = element_tangent(coords, u, conn, lam, mu, W)
    if skip is not None:
        Ke = Ke * (~skip).to(F64)[:, None, None]
    nn = coords.shape[0]
    dof = (2 * conn[:, :, None] + torch.arange(2)[None, None, :]).reshape(-1, 6)               # [Ne, 6]
    K = torch.zeros(2 * nn, 2 * nn, dtype=F64)
    K.index_put_((dof[:, :, None].expand(-1, 6, 6).reshape(-1), dof[:, None, :].expand(-1, 6, 6).reshape(-1)), Ke.reshape(-1),
                 accumulate=True)
    return K


def free_dofs(free):
    """The dof indices of the free nodes (bool mask [Nn]), node-major."""
    n = torch.nonzero(free)[:, 0]
    return (2 * n[:, None] + torch.arange(2)[None, :]).reshape(-1)


def restrict(K, free):
    d = free_dofs(free)
    return K[d][:, d]


def diag_blocks(Kff):
    """-> [n, 3] = {K_xx, K_xy, K_yy} of every free node's 2 x 2 diagonal block."""
    n = Kff.shape[0] // 2
    i = 2 * torch.arange(n)
    return torch.stack([Kff[i, i], 0.5 * (Kff[i, i + 1] + Kff[i + 1, i]), Kff[i + 1, i + 1]], dim=1)


def jacobi_inverse(blocks):
    """The inverse blocks [n, 3]; the identity for a block that is not positive definite."""
    a, b, c = blocks[:, 0], blocks[:, 1], blocks[:, 2]
    det = a * c - b * b
    pd = (det > 0) & (a > 0) & torch.isfinite(det)
    safe = torch.where(pd, det, torch.ones_like(det))
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    return torch.stack([torch.where(pd, c / safe, one), torch.where(pd, -b / safe, zero), torch.where(pd, a / safe, one)], dim=1), pd


def apply_blocks(dinv, r):
    """z = M r for r [n, 2]."""
    return torch.stack([dinv[:, 0] * r[:, 0] + dinv[:, 1] * r[:, 1], dinv[:, 1] * r[:, 0] + dinv[:, 2] * r[:, 1]], dim=1)


# ---------------------------------------------------------------- the problem: energy with edges over the free rows
class Problem:
    """One mesh with Dirichlet rows ``bc`` (values ``u_fixed`` [n_fixed, 2]) and dead edge loads ``T`` over ``edges``; the
    unknowns are the free rows in node order."""

    def __init__(self, coords, conn, bc, u_fixed, lam, mu, W, edges=None, T=None):
        self.coords, self.conn, self.bc = coords, conn, bc
        self.free = ~bc
        self.u_fixed = torch.zeros(int(bc.sum()), 2, dtype=F64) if u_fixed is None else u_fixed
        self.lam, self.mu, self.W, self.edges, self.T = lam, mu, W, edges, T
        self.n = int(self.free.sum())

    def full(self, uf):
        u = torch.zeros(self.coords.shape[0], 2, dtype=F64)
        u[self.free] = uf
        u[self.bc] = self.u_fixed
        return u

    def energy(self, uf):
        """-> (Pi, g [n, 2], min J, inverted count)"""
        r = H.total(self.coords, self.full(uf), self.conn, self.lam, self.mu, self.W, None, self.edges, self.T)
        return r["loss"], r["gU"][self.free], r["min_J"], r["count"]

    def tangent(self, uf):
        return restrict(dense_tangent(self.coords, self.full(uf), self.conn, self.lam, self.mu, self.W), self.free)


# ---------------------------------------------------------------- truncated PCG, the device driver's recursion
def pcg(K, dinv, g, eta, max_iter):
    """K d = -g from d = 0: stops at |r| <= eta |g| ("rtol"), at ``max_iter`` ("max_iter") or where p^T K p <= 0
    ("breakdown", detected before d moves).  -> (d [n, 2], iterations, reason)"""
    n = g.shape[0]
    d = torch.zeros_like(g)
    r = -g.clone()
    z = apply_blocks(dinv, r)
    rho = (r * z).sum()
    tol = eta * g.norm()
    p = torch.zeros_like(g)
    beta = 0.0
    it = 0
    if r.norm() <= tol:
        return d, 0, "rtol"
    if max_iter <= 0:
        return d, 0, "max_iter"
    while True:
        p = z + beta * p
        q = (K @ p.reshape(-1)).reshape(n, 2)
        pq = (p * q).sum()
        alpha = rho / pq
        if not (pq > 0) or not torch.isfinite(alpha):
            return d, it, "breakdown"
        d = d + alpha * p
        r = r - alpha * q
        z = apply_blocks(dinv, r)
        rho_new = (r * z).sum()
        beta = rho_new / rho
        rho = rho_new
        it += 1
        if r.norm() <= tol:
            return d, it, "rtol"
        if it >= max_iter:
            return d, it, "max_iter"


@dataclass
class Result:
    u: torch.Tensor
    newton_iterations: int = 0
    cg_iterations: int = 0
    grad_norm: float = 0.0
    rhs_norm: float = 0.0
    energy: float = 0.0
    min_J: float = 0.0
    converged: bool = False
    reason: str = ""
    history: list = _field(default_factory=list)


def newton(prob, u0, rtol=1e-8, atol=0.0, max_newton=50, cg_max_iter=None, eta_max=0.1, armijo=1e-4, max_backtracks=30):
    """Inexact Newton on ``prob`` from the free rows ``u0``.  ``history``: one dict per Newton iteration (energy and |g| at its
    start, eta, cg iterations and halt reason, the accepted step t, min J of the accepted state)."""
    u = u0.clone()
    cg_max_iter = max(1000, 4 * prob.n) if cg_max_iter is None else cg_max_iter
    rhs = prob.energy(torch.zeros_like(u))[1].norm().item()
    tol = max(rtol * rhs, atol)
    E, g, min_j, count = prob.energy(u)
    res = Result(u=u, rhs_norm=rhs, energy=E, min_J=min_j, grad_norm=g.norm().item())
    if count > 0:
        res.reason = "inverted"
        return res
    gn_prev = None
    k = 0
    while True:
        gn = g.norm().item()
        res.grad_norm, res.energy, res.min_J, res.newton_iterations = gn, E, min_j, k
        if gn <= tol:
            res.converged, res.reason = True, "rtol" if rtol * rhs >= atol else "atol"
            break
        if k >= max_newton:
            res.reason = "max_newton"
            break
        eta = eta_max if gn_prev is None else min(max(0.9 * (gn / gn_prev) ** 2, 1e-12), eta_max)
        K = prob.tangent(u)
        dinv, _ = jacobi_inverse(diag_blocks(K))
        d, its, halt = pcg(K, dinv, g, eta, cg_max_iter)
        if halt == "breakdown" and its == 0:
            d = -apply_blocks(dinv, g)
        res.cg_iterations += its
        gtd = (g * d).sum().item()
        t, accepted = 1.0, False
        for _ in range(max_backtracks + 1):
            Et, gt, mj, cnt = prob.energy(u + t * d)
            if Et == Et and abs(Et) != float("inf") and Et <= E + armijo * t * gtd + 4 * EPS * abs(E):
                accepted = True
                break
            t *= 0.5
        entry = dict(energy=E, grad_norm=gn, eta=eta, cg_iterations=its, cg_reason=halt, step=t if accepted else 0.0, min_J=min_j)
        res.history.append(entry)
        if not accepted:
            res.reason = "line_search"
            break
        u = u + t * d
        gn_prev = gn
        E, g, min_j = Et, gt, mj
        entry["min_J"] = mj
        k += 1
    res.u = u
    return res


# ---------------------------------------------------------------- the three runs of the tests
E_SOFT = 2e6


def plate_problem(traction=None, loads=True):
    """The 17 x 9 plate, E = 2e6, left edge clamped (u = 0); ``traction``: a constant (tx, ty) on the right edge (None: the
    default (1e5, 0)); ``loads=False``: no edge loads at all."""
    coords, conn, _, bc, _, edges = H.meshes()["plate"]
    lam, mu = H.lame(E=E_SOFT)
    t = None
    if traction is not None:
        tx, ty = traction
        t = lambda x: torch.stack([torch.full_like(x[:, 0], tx), torch.full_like(x[:, 0], ty)], dim=1)
    T = H.traction_table(coords, edges, t) if loads else None
    return Problem(coords, conn, bc, None, lam, mu, H.tri_W(), edges if loads else None, T)


RUNS = {
    # name: (traction, loads, start, caps (newton, cg))
    "default": (None, True, "zero", (10, 1000)),
    "down": ((0.0, -4e4), True, "zero", (15, 2000)),
    "relax": (None, False, "field", (20, 2000)),
}


def run_start(prob, start):
    if start == "zero":
        return torch.zeros(prob.n, 2, dtype=F64)
    return H.field(prob.coords)[prob.free].clone()                 # the clamped rows are zero in the problem


_runs = {}


def reference_run(name):
    """-> (problem, Result, ||g|| at the start) of one of RUNS, computed once.  Loaded runs stop at rtol = 1e-10; without loads
    ||g(u_free = 0)|| is identically 0, so the start's gradient norm takes its place through atol = 1e-10 ||g(start)||."""
    if name not in _runs:
        traction, loads, start, _ = RUNS[name]
        prob = plate_problem(traction, loads)
        u0 = run_start(prob, start)
        g_start = prob.energy(u0)[1].norm().item()
        kw = dict(rtol=1e-10) if loads else dict(rtol=0.0, atol=1e-10 * g_start)
        _runs[name] = (prob, newton(prob, u0, **kw), g_start)
    return _runs[name]
