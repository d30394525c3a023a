"""CPU-torch fp64 statement of the QUAD4 Neo-Hookean tangent and of the inexact Newton solve on it, shared by the
tests (a plain helper module, not a conftest).  It imports ``quad4_hyper_reference`` and ``newton_reference`` and nothing
from the library's compute paths: the PCG recursion, the Newton driver, the block-Jacobi helpers and the three runs are
``newton_reference``'s, unchanged, on a problem of this module.

Per cell and Gauss point q, in ``quad4_hyper_reference``'s notation (J_q, H_q = G_q J_q^-1, L_q = log1p(j_q), T_q = F_q^-T,
A_q = |det J_q|), for a direction p on the four corners with dG_q = sum_k p_k (x) grad_xi N_k(xi_q):

    dH = dG J^-1
    dP = mu dH + (mu - lambda L) T dH^T T + lambda (T : dH) T
    q_k = sum_q A_q dP_q J_q^-T grad_xi N_k(xi_q)

Dead loads do not enter.  A cell with j_q <= -1 (or NaN) at any point contributes a zero 8 x 8 block.  The corner blocks in
closed form, with w = J_q^-T grad_xi N_a(xi_q) and t = T_q w:

    K_aa = sum_q A_q [mu |w|^2 I + (mu - lambda L + lambda) t (x) t]
"""
import torch

import newton_reference as N
import quad4_hyper_reference as Q

F64 = torch.float64


# ---------------------------------------------------------------- the tangent
def _state(coords, u, conn, lam, mu):
    X, U = coords[conn], u[conn]
    Jm = torch.einsum("eki,qjk->eqij", X, Q.DN)
    G = torch.einsum("eki,qjk->eqij", U, Q.DN)
    Jinv, det = Q._inv2(Jm)
    H = G @ Jinv
    j = H[..., 0, 0] + H[..., 1, 1] + (H[..., 0, 0] * H[..., 1, 1] - H[..., 0, 1] * H[..., 1, 0])
    bad = ~(j > -1.0)
    inverted = bad.any(dim=1)
    js = torch.where(bad, torch.zeros_like(j), j)
    L = torch.log1p(js)
    F = torch.eye(2, dtype=F64) + H
    T = torch.stack([torch.stack([F[..., 1, 1], -F[..., 1, 0]], -1), torch.stack([-F[..., 0, 1], F[..., 0, 0]], -1)], -2) \
        / (1.0 + js)[..., None, None]
    A = det.abs() * (~inverted).to(F64)[:, None]
    return Jinv, T, L, A, 1.0 + j, inverted


def element_tangent(coords, u, conn, lam, mu):
    """-> Ke [Ne, 8, 8] over the dofs (corner k, component c) -> 2 k + c; zero for an inverted cell."""
    Jinv, T, L, A, _, _ = _state(coords, u, conn, lam, mu)
    ne = conn.shape[0]
    c = mu - lam * L
    JinvT = Jinv.transpose(-1, -2)
    Ke = torch.zeros(ne, 8, 8, dtype=F64)
    for l in range(4):
        for comp in range(2):
            dG = torch.zeros(ne, 4, 2, 2, dtype=F64)
            dG[:, :, comp, :] = Q.DN[None, :, :, l]
            dH = dG @ Jinv
            tdh = (T * dH).sum(dim=(-1, -2))
            dP = mu * dH + c[..., None, None] * (T @ dH.transpose(-1, -2) @ T) + (lam * tdh)[..., None, None] * T
            Qm = A[..., None, None] * (dP @ JinvT)
            Ke[:, :, 2 * l + comp] = torch.einsum("eqij,qjk->eki", Qm, Q.DN).reshape(ne, 8)
    return Ke


def corner_blocks(coords, u, conn, lam, mu):
    """The closed form -> [Ne, 4, 3] = {K_xx, K_xy, K_yy} of every corner's 2 x 2 diagonal block; zero for an inverted cell."""
    Jinv, T, L, A, _, _ = _state(coords, u, conn, lam, mu)
    w = torch.einsum("eqji,qjk->eqki", Jinv, Q.DN)                 # w[k] = J^-T grad N_k
    t = torch.einsum("eqij,eqkj->eqki", T, w)
    ww = (w * w).sum(-1)                                           # [Ne, q, k]
    c = (mu - lam * L + lam)[..., None]
    xx = (A[..., None] * (mu * ww + c * t[..., 0] * t[..., 0])).sum(1)
    xy = (A[..., None] * (c * t[..., 0] * t[..., 1])).sum(1)
    yy = (A[..., None] * (mu * ww + c * t[..., 1] * t[..., 1])).sum(1)
    return torch.stack([xx, xy, yy], dim=-1)


def unit_blocks(Ke):
    """The corner blocks read off the 8 x 8 tangents -> [Ne, 4, 3]."""
    return torch.stack([torch.stack([Ke[:, 2 * a, 2 * a], 0.5 * (Ke[:, 2 * a, 2 * a + 1] + Ke[:, 2 * a + 1, 2 * a]),
                                     Ke[:, 2 * a + 1, 2 * a + 1]], dim=1) for a in range(4)], dim=1)


def dense_tangent(coords, u, conn, lam, mu, skip=None):
    """K_T [2 Nn, 2 Nn] (dof 2 n + c).  ``skip``: a bool mask [Ne] of cells left out."""
    Ke = element_tangent(coords, u, conn, lam, mu)
    if skip is not None:
        Ke = Ke * (~skip).to(F64)[:, None, None]
    nn = coords.shape[0]
    dof = (2 * conn[:, :, None] + torch.arange(2)[None, None, :]).reshape(-1, 8)
    K = torch.zeros(2 * nn, 2 * nn, dtype=F64)
    K.index_put_((dof[:, :, None].expand(-1, 8, 8).reshape(-1), dof[:, None, :].expand(-1, 8, 8).reshape(-1)), Ke.reshape(-1),
                 accumulate=True)
    return K


# ---------------------------------------------------------------- the problem newton_reference's driver runs on
class Problem:
    """``newton_reference.Problem`` for cells: Dirichlet rows ``bc`` (values ``u_fixed``), dead edge loads ``T`` over
    ``edges``; the unknowns are the free rows in node order."""

    def __init__(self, coords, conn, bc, u_fixed, lam, mu, edges=None, T=None):
        self.coords, self.conn, self.bc = coords, conn, bc
        self.free = ~bc
        self.u_fixed = torch.zeros(int(bc.sum()), 2, dtype=F64) if u_fixed is None else u_fixed
        self.lam, self.mu, self.edges, self.T = lam, mu, edges, T
        self.n = int(self.free.sum())

    def full(self, uf):
        u = torch.zeros(self.coords.shape[0], 2, dtype=F64)
        u[self.free] = uf
        u[self.bc] = self.u_fixed
        return u

    def energy(self, uf):
        """-> (Pi, g [n, 2], min J, inverted count)"""
        r = Q.total(self.coords, self.full(uf), self.conn, self.lam, self.mu, None, self.edges, self.T)
        return r["loss"], r["gU"][self.free], r["min_J"], r["count"]

    def tangent(self, uf):
        return N.restrict(dense_tangent(self.coords, self.full(uf), self.conn, self.lam, self.mu), self.free)


def plate_problem(traction=None, loads=True):
    """``newton_reference.plate_problem`` on the QUAD4 17 x 9 plate: E = ``N.E_SOFT``, left edge clamped at 0."""
    coords, conn, _, bc, _, edges = Q.meshes()["plate"]
    lam, mu = Q.lame(E=N.E_SOFT)
    t = None
    if traction is not None:
        tx, ty = traction
        t = lambda x: torch.stack([torch.full_like(x[:, 0], tx), torch.full_like(x[:, 0], ty)], dim=1)
    T = Q.traction_table(coords, edges, t) if loads else None
    return Problem(coords, conn, bc, None, lam, mu, edges if loads else None, T)


def run_start(prob, start):
    if start == "zero":
        return torch.zeros(prob.n, 2, dtype=F64)
    return Q.field(prob.coords)[prob.free].clone()


_runs = {}


def reference_run(name):
    """-> (problem, Result, ||g|| at the start) of one of ``N.RUNS`` on the QUAD4 plate, computed once; the stopping rules are
    ``newton_reference.reference_run``'s."""
    if name not in _runs:
        traction, loads, start, _ = N.RUNS[name]
        prob = plate_problem(traction, loads)
        u0 = run_start(prob, start)
        g_start = prob.energy(u0)[1].norm().item()
        kw = dict(rtol=1e-10) if loads else dict(rtol=0.0, atol=1e-10 * g_start)
        _runs[name] = (prob, N.newton(prob, u0, **kw), g_start)
    return _runs[name]
