"""CPU-torch fp64 statement of the Cauchy stress recovery and the ZZ indicator at finite strain, shared by the
tests (a plain helper module, not a conftest).  Written independently of the device formulas: the stress comes from autograd,

    P = d psi / d F  of ``hyper_reference.psi_of_F`` (the textbook energy),   sigma_h = P F^T / det F  ->  (sxx, syy, sxy)

at the points of ``zz_reference`` (TRI3 the centroid with w = |det Jg| / 2, QUAD4 the 2x2 Gauss points with w_q = |det J_q|, on
the reference configuration), with F = I + G J^-1 the deformation gradient there.  Then, as ``zz_reference``:

    sigma*_n = sum w_q N_n(q) sigma_h(q) / sum w_q N_n(q),   J*_n = the same projection of det F
    eta_e^2 = int_e (sigma* - sigma_h).S.(sigma* - sigma_h) dX,   |sigma_h|_e^2 = int_e sigma_h.S.sigma_h dX,   S = C0^-1
    C0 = [[lambda + 2 mu, lambda, 0], [lambda, lambda + 2 mu, 0], [0, 0, mu]]      (the material linearised at F = I)
    relative = sqrt(eta^2 / (|sigma_h|^2 + eta^2))

Inverted elements (det F <= 0 or NaN at any point): weight 0 in the projection, eta_e^2 = +inf, 0 to |sigma_h|^2; a node with
no other element gets zeros and area 0; ``relative`` = 1.0; min_J is the minimum of det F over all points.  (Their points are
evaluated at F = I here: the values are masked everywhere, only no NaN may come out of them.)
"""
import torch

import hyper_reference as H
import quad4_hyper_reference as Q4
import zz_reference as Z

F64 = torch.float64

meshes = Z.meshes
field, patch_field, rotate_field = H.field, H.patch_field, H.rotate_field
invert_one_element, invert_one_cell = H.invert_one_element, Q4.invert_one_cell


def C0(lam, mu):
    return torch.tensor([[lam + 2 * mu, lam, 0.0], [lam, lam + 2 * mu, 0.0], [0.0, 0.0, mu]], dtype=F64)


def deformation_gradients(coords, u, conn):
    """-> (F [Ne, NQ, 2, 2], |det J| [Ne, NQ]) at the element points."""
    if conn.shape[1] == 3:
        _, _, Jg, G = H._parts(coords, u, conn)
        Jm, G = Jg[:, None], G[:, None]
    else:
        Jm = torch.einsum("eki,qjk->eqij", coords[conn], Q4.DN)
        G = torch.einsum("eki,qjk->eqij", u[conn], Q4.DN)
    F = torch.eye(2, dtype=F64) + G @ torch.linalg.inv(Jm)
    return F, torch.linalg.det(Jm).abs()


def cauchy_autograd(F, lam, mu):
    """sigma = P F^T / det F with P = d psi_of_F / dF by autograd; F [..., 2, 2] -> [..., 3] = (sxx, syy, sxy)."""
    flat = F.reshape(-1, 2, 2)
    P = torch.func.vmap(torch.func.grad(lambda f: H.psi_of_F(f, lam, mu)))(flat)
    s = P @ flat.transpose(1, 2) / torch.linalg.det(flat)[:, None, None]
    return torch.stack([s[:, 0, 0], s[:, 1, 1], 0.5 * (s[:, 0, 1] + s[:, 1, 0])], dim=1).reshape(F.shape[:-2] + (3,))


def cauchy_closed(F, lam, mu):
    """The issue's cancellation-free closed form (mu (H + H^T + H H^T) + lambda log1p(j) I) / (1 + j), for comparison."""
    Hm = F - torch.eye(2, dtype=F64)
    j = Hm[..., 0, 0] + Hm[..., 1, 1] + (Hm[..., 0, 0] * Hm[..., 1, 1] - Hm[..., 0, 1] * Hm[..., 1, 0])
    B = Hm + Hm.transpose(-1, -2) + Hm @ Hm.transpose(-1, -2)
    s = (mu * B + (lam * torch.log1p(j))[..., None, None] * torch.eye(2, dtype=F64)) / (1.0 + j)[..., None, None]
    return torch.stack([s[..., 0, 0], s[..., 1, 1], s[..., 0, 1]], dim=-1)


def point_terms(coords, u, conn, lam, mu, stress=cauchy_autograd):
    """-> dict(sig [Ne, NQ, 3], J [Ne, NQ] = det F (true values), w [Ne, NQ] (unmasked), inverted [Ne] bool)."""
    F, adet = deformation_gradients(coords, u, conn)
    J = torch.linalg.det(F)
    bad = ~(J > 0.0)
    Fs = torch.where(bad[..., None, None], torch.eye(2, dtype=F64).expand_as(F), F)
    _, wf = Z.points(conn.shape[1])
    return dict(sig=stress(Fs, lam, mu), J=J, w=adet * wf[None, :], inverted=bad.any(dim=1))


def recover(coords, u, conn, lam, mu, pt=None):
    """-> (sigma* [Nn, 3], J* [Nn], lumped nodal area [Nn])."""
    npe, nn = conn.shape[1], coords.shape[0]
    pt = point_terms(coords, u, conn, lam, mu) if pt is None else pt
    w = torch.where(pt["inverted"][:, None], torch.zeros_like(pt["w"]), pt["w"])
    Jm = torch.where(pt["inverted"][:, None], torch.ones_like(pt["J"]), pt["J"])
    N = Z.shape_table(npe, Z.points(npe)[0])                           # [NQ, npe]
    wn = w[:, :, None] * N[None, :, :]                                 # [Ne, NQ, npe]
    vals = torch.cat([pt["sig"], Jm[:, :, None]], dim=2)               # [Ne, NQ, 4]
    num_e = torch.einsum("eqk,eqi->eki", wn, vals)
    den_e = wn.sum(dim=1)
    num = torch.zeros(nn, 4, dtype=F64).index_add_(0, conn.reshape(-1), num_e.reshape(-1, 4))
    den = torch.zeros(nn, dtype=F64).index_add_(0, conn.reshape(-1), den_e.reshape(-1))
    out = torch.where(den[:, None] > 0, num / den[:, None].clamp_min(1e-300), torch.zeros_like(num))
    return out[:, :3], out[:, 3], den


def zz(coords, u, conn, lam, mu, tri_rule="closed", stress=cauchy_autograd):
    """-> dict(nodal_stress, nodal_J, area, sig_h [Ne, NQ, 3], J [Ne, NQ], eta2 [Ne], norm2 [Ne], eta2_total, norm2_total, eta,
    relative, min_J, inverted (count), inverted_mask)."""
    npe = conn.shape[1]
    S = torch.linalg.inv(C0(lam, mu))
    pt = point_terms(coords, u, conn, lam, mu, stress)
    sig_star, J_star, area = recover(coords, u, conn, lam, mu, pt)
    sig, w, inv = pt["sig"], pt["w"], pt["inverted"]
    norm2 = (w * Z._s_form(S, sig)).sum(dim=1)
    ss = sig_star[conn]
    if npe == 3 and tri_rule == "closed":
        d = ss - sig[:, 0:1, :]
        eta2 = w[:, 0] / 12.0 * (Z._s_form(S, d).sum(dim=1) + Z._s_form(S, d.sum(dim=1)))
    else:
        if npe == 3:
            epts = torch.tensor([[1 / 6, 1 / 6], [2 / 3, 1 / 6], [1 / 6, 2 / 3]], dtype=F64)
            ew, esig = (w[:, 0:1] / 3.0).expand(-1, 3), sig.expand(-1, 3, -1)
        else:
            epts, ew, esig = Z.points(4)[0], w, sig
        d = torch.einsum("qk,eki->eqi", Z.shape_table(npe, epts), ss) - esig
        eta2 = (ew * Z._s_form(S, d)).sum(dim=1)
    eta2 = torch.where(inv, torch.full_like(eta2, float("inf")), eta2)
    norm2 = torch.where(inv, torch.zeros_like(norm2), norm2)
    e2, n2, count = eta2.sum().item(), norm2.sum().item(), int(inv.sum().item())
    J = pt["J"]
    rel = 1.0 if count > 0 else ((e2 / (n2 + e2)) ** 0.5 if n2 + e2 > 0 else 0.0)
    return dict(nodal_stress=sig_star, nodal_J=J_star, area=area, sig_h=sig, J=J, eta2=eta2, norm2=norm2, eta2_total=e2,
                norm2_total=n2, eta=e2 ** 0.5, relative=rel, min_J=J[~torch.isnan(J)].min().item(), inverted=count,
                inverted_mask=inv)


def von_mises(s):
    return torch.sqrt(s[:, 0] ** 2 - s[:, 0] * s[:, 1] + s[:, 1] ** 2 + 3.0 * s[:, 2] ** 2)
