"""CPU-torch fp64 statement of the compressible Neo-Hookean QUAD4 total potential, shared by the tests (a plain
helper module, not a conftest).  It imports nothing from the library's compute paths (meshes come from the generators and
``tests/quad_meshes.py``); material, fields, edge terms and the traction table are ``tests/hyper_reference.py``'s.

Per cell, corners counter-clockwise from (-1, -1) (a clockwise cell works: |det J|), at the 2x2 Gauss points
xi_q = (+-1/sqrt(3), +-1/sqrt(3)) in the order (-,-) (+,-) (-,+) (+,+), weights 1:

    J_q = sum_k X_k (x) grad_xi N_k(xi_q),  G_q = sum_k U_k (x) grad_xi N_k(xi_q),  H_q = G_q J_q^-1
    j_q = tr H_q + det H_q (= det F_q - 1),  L_q = log1p(j_q)
    psi_q = mu (tr H_q + H_q:H_q / 2 - L_q) + lambda L_q^2 / 2
    P_q = mu (H_q + H_q^T F_q^-T) + lambda L_q F_q^-T
    e = sum_q |det J_q| (psi_q - b_q . u_h(xi_q))
    de/dG_q = |det J_q| P_q J_q^-T,   de/dJ_q = |det J_q| ((psi_q - b_q . u_h) I - H_q^T P_q) J_q^-T
    spread to corner k through grad_xi N_k(xi_q);  -|det J_q| N_k(xi_q) b_q joins de/dU_k

A cell with j_q <= -1 (or NaN) at any point has energy +inf and zero gradient contributions; it is counted once (each such
point is evaluated at j = 0).  min J is the minimum of 1 + j_q over all points.  Neumann edges are dead loads
(``hyper_reference.edge_terms``).
"""
import math

import numpy as np
import torch

from hyper_reference import F0, edge_terms, field, lame, patch_field, psi_of_F, rotate_field, traction_table  # noqa: F401

F64 = torch.float64
GP = 1.0 / math.sqrt(3.0)
XI = torch.tensor([-1.0, 1.0, 1.0, -1.0], dtype=F64)                 # corners
ETA = torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=F64)
PTS = torch.tensor([[-GP, -GP], [GP, -GP], [-GP, GP], [GP, GP]], dtype=F64)
N = 0.25 * (1 + XI[None, :] * PTS[:, 0:1]) * (1 + ETA[None, :] * PTS[:, 1:2])                    # [q, k]
DN = torch.stack([0.25 * XI[None, :] * (1 + ETA[None, :] * PTS[:, 1:2]),
                  0.25 * ETA[None, :] * (1 + XI[None, :] * PTS[:, 0:1])], dim=1)                 # [q, j, k]

JITTER, SEED = 0.3, 4                                                # min J of `field` > 0.2 on every mesh (asserted)


def meshes():
    """name -> mesh 6-tuple (fp64), all on [0, 2] x [0, 1]."""
    import quad_meshes as QM
    from hidenn_fem_amd.mesh import structured_quad_mesh
    split = QM.split_tri_quads(150)
    return {
        "jittered": structured_quad_mesh(17, 9, jitter=JITTER, seed=SEED, dtype=F64),
        "split": split,
        "mixed": QM.renumber(split, seed=11, orient="mixed")[0],
        "plate": structured_quad_mesh(17, 9, dtype=F64),
    }


def body_points(b_force):
    """b at the four Gauss points of the reference square [4, 2] (EnergyLoss2D._quad4_body's table)."""
    return b_force(PTS).to(F64)


def _inv2(M):
    det = M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 1, 0]
    adj = torch.stack([torch.stack([M[..., 1, 1], -M[..., 0, 1]], -1), torch.stack([-M[..., 1, 0], M[..., 0, 0]], -1)], -2)
    return adj / det[..., None, None], det


def element_terms(coords, u, conn, lam, mu, Bq=None):
    """-> dict(e [Ne] (inf where inverted), J [Ne, 4] = 1 + j_q, gX [Ne, 4, 2], gU [Ne, 4, 2], inverted [Ne] bool)."""
    X, U = coords[conn], u[conn]                                   # [Ne, 4, 2]
    Bq = torch.zeros(4, 2, dtype=F64) if Bq is None else torch.as_tensor(Bq, dtype=F64).reshape(4, 2)
    Jm = torch.einsum("eki,qjk->eqij", X, DN)                      # J[i][j] = sum_k X_k[i] dN_k/dxi_j
    G = torch.einsum("eki,qjk->eqij", U, DN)
    Jinv, det = _inv2(Jm)
    H = G @ Jinv
    tr = H[..., 0, 0] + H[..., 1, 1]
    j = tr + (H[..., 0, 0] * H[..., 1, 1] - H[..., 0, 1] * H[..., 1, 0])
    bad = ~(j > -1.0)                                              # [Ne, 4]
    inverted = bad.any(dim=1)
    js = torch.where(bad, torch.zeros_like(j), j)
    L = torch.log1p(js)
    psi = mu * (tr + 0.5 * (H * H).sum(dim=(-1, -2)) - L) + 0.5 * lam * L * L
    I = torch.eye(2, dtype=F64)
    F = I + H
    FinvT = torch.stack([torch.stack([F[..., 1, 1], -F[..., 1, 0]], -1), torch.stack([-F[..., 0, 1], F[..., 0, 0]], -1)], -2) \
        / (1.0 + js)[..., None, None]
    P = mu * (H + H.transpose(-1, -2) @ FinvT) + (lam * L)[..., None, None] * FinvT
    ad = det.abs()
    uh = torch.einsum("qk,eki->eqi", N, U)
    w = psi - (uh * Bq[None]).sum(-1)                              # psi - b . u_h
    e = (ad * w).sum(dim=1)
    JinvT = Jinv.transpose(-1, -2)
    dG = ad[..., None, None] * (P @ JinvT)
    dJ = ad[..., None, None] * ((w[..., None, None] * I - H.transpose(-1, -2) @ P) @ JinvT)
    gU = torch.einsum("eqij,qjk->eki", dG, DN) - torch.einsum("eq,qk,qi->eki", ad, N, Bq)
    gX = torch.einsum("eqij,qjk->eki", dJ, DN)
    zero = torch.zeros_like(gX)
    keep = (~inverted)[:, None, None]
    return dict(e=torch.where(inverted, torch.full_like(e, float("inf")), e), J=1.0 + j, gX=torch.where(keep, gX, zero),
                gU=torch.where(keep, gU, zero), inverted=inverted)


def total(coords, u, conn, lam, mu, Bq=None, edges=None, T=None):
    """-> dict(loss (python float, inf when a cell is inverted), gX [Nn, 2], gU [Nn, 2] by node id, min_J, count)."""
    t = element_terms(coords, u, conn, lam, mu, Bq)
    nn = coords.shape[0]
    gX = torch.zeros(nn, 2, dtype=F64).index_add_(0, conn.reshape(-1), t["gX"].reshape(-1, 2))
    gU = torch.zeros(nn, 2, dtype=F64).index_add_(0, conn.reshape(-1), t["gU"].reshape(-1, 2))
    loss = t["e"].sum()
    if edges is not None and edges.shape[0] > 0:
        T = torch.as_tensor(T, dtype=F64)
        T = T.reshape(1, 4).expand(edges.shape[0], 4) if T.numel() == 4 else T
        w, eX, eU = edge_terms(coords, u, edges, T)
        loss = loss - w.sum()
        gX.index_add_(0, edges.reshape(-1), eX.reshape(-1, 2))
        gU.index_add_(0, edges.reshape(-1), eU.reshape(-1, 2))
    return dict(loss=loss.item(), gX=gX, gU=gU, min_J=t["J"].min().item(), count=int(t["inverted"].sum().item()))


def naive_total(coords, u, conn, lam, mu):
    """The textbook statement through autograd: sum_e sum_q |det J_q| (mu/2 (tr F^T F - 2) - mu ln J + lambda/2 ln^2 J)
    -> (loss, gX, gU) by node id.  Loses accuracy as 1e-16 / strain^2: a checker for finite strains only."""
    x = coords.clone().requires_grad_(True)
    v = u.clone().requires_grad_(True)
    Jm = torch.einsum("eki,qjk->eqij", x[conn], DN)
    G = torch.einsum("eki,qjk->eqij", v[conn], DN)
    F = torch.eye(2, dtype=F64) + G @ torch.linalg.inv(Jm)
    J = torch.linalg.det(F)
    psi = 0.5 * mu * ((F * F).sum(dim=(-1, -2)) - 2.0) - mu * torch.log(J) + 0.5 * lam * torch.log(J) ** 2
    loss = (torch.linalg.det(Jm).abs() * psi).sum()
    loss.backward()
    return loss.item(), x.grad, v.grad


def area(coords, conn):
    """Sum of the cells' areas (shoelace; either orientation)."""
    X = coords[conn]
    d1, d2 = X[:, 2] - X[:, 0], X[:, 3] - X[:, 1]
    return 0.5 * (d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]).abs().sum().item()


def linear_physical(coords, u, conn, E=10e9, nu=0.3):
    """The small-strain QUAD4 energy in the physical convention and its gradients by node id, from the oracle."""
    from oracle import quad4 as Q, ref_chain as R
    x = coords.clone().requires_grad_(True)
    v = u.clone().requires_grad_(True)
    loss = Q.quad4_domain_energy(x, v, conn, R.plane_stress_C(E, nu).to(F64), None, convention="physical")
    loss.backward()
    return loss.item(), x.grad, v.grad


def invert_one_cell(coords, u, conn):
    """A copy of ``u`` with one interior node moved so that exactly one cell is inverted (asserted by the caller on
    ``total``): ``invert_one_element``'s construction for cells -- the node is pushed across the diagonal through its two
    neighbours in one of its cells, by the smallest push found (det F is checked at the Gauss points, not at the corner, so
    the push has to go well past the diagonal)."""
    x = coords + u
    on_boundary = (coords[:, 0] < 1e-9) | (coords[:, 0] > 2 - 1e-9) | (coords[:, 1] < 1e-9) | (coords[:, 1] > 1 - 1e-9)
    lam, mu = lame()
    for push in (1.15, 1.5, 2.0, 2.5):
        for e in range(conn.shape[0]):
            for c in range(4):
                n = int(conn[e, c])
                if on_boundary[n]:
                    continue
                p, q = x[conn[e, (c + 1) % 4]], x[conn[e, (c + 3) % 4]]
                foot = p + (q - p) * ((x[n] - p) @ (q - p)) / ((q - p) @ (q - p))
                v = u.clone()
                v[n] = u[n] + push * (foot - x[n])
                if total(coords, v, conn, lam, mu)["count"] == 1:
                    return v, n
    raise RuntimeError("no single-cell inversion found")
