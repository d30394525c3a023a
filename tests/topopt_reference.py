"""numpy / scipy statement of element-scaled stiffness and SIMP compliance topology optimisation, shared by the
topopt tests (a plain helper module, not a conftest).  Independent of the kernels' text:

    K_e            per element from ``buckling_reference.element_points`` (the points, weights and gradients of the definition)
    K(w)           sparse sum_e w_e K_e over the free u rows in a given row order
    F              the density filter as a dense matrix, by brute force over all pairs:
                   F_ej = H_ej v_j / s_e,  H_ej = max(0, r - |x_e - x_j|),  s_e = sum_j H_ej v_j
    OC             rho_new,e(lam) = clamp(rho_e sqrt(max(0, -dc_e / dv_e) / lam), max(0, rho_e - move), min(1, rho_e + move))
                   and the bisection with the device's rule (``oc_bisect``)
    sensitivity    dc/drho = F^T (-penal rho~^(penal-1) (1 - e_min) u_e^T K_e u_e)
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import buckling_reference as BR


def element_matrices(coords, conn, mat, W, convention):
    """[ne, 2 npe, 2 npe] K_e (dofs interleaved (x, y) per corner)."""
    coords, conn = np.asarray(coords, dtype=np.float64), np.asarray(conn, dtype=np.int64)
    Cm = BR.material(mat)
    npe = conn.shape[1]
    out = np.zeros((conn.shape[0], 2 * npe, 2 * npe))
    for e, nd in enumerate(conn):
        for g, w in BR.element_points(coords[nd], convention, W):
            B = np.zeros((3, 2 * npe))
            B[0, 0::2], B[1, 1::2] = g[0], g[1]
            B[2, 0::2], B[2, 1::2] = g[1], g[0]
            out[e] += w * (B.T @ Cm @ B)
    return out


def element_dofs(conn, node_row):
    """[ne, 2 npe] free dof of every element dof (2 row + c), -1 on a Dirichlet node; ``node_row[n]`` = free row or -1."""
    r = np.asarray(node_row, dtype=np.int64)[np.asarray(conn, dtype=np.int64)]
    d = np.stack([2 * r, 2 * r + 1], axis=2).reshape(conn.shape[0], -1)
    d[np.repeat(r < 0, 2, axis=1)] = -1
    return d


def node_rows(row_node, n_nodes):
    out = -np.ones(n_nodes, dtype=np.int64)
    out[np.asarray(row_node, dtype=np.int64)] = np.arange(len(row_node))
    return out


def scaled_stiffness(Ke, dofs, w, n_free):
    """Sparse K(w)_ff = sum_e w_e K_e over the free dofs (CSR)."""
    m = Ke.shape[1]
    i = np.repeat(dofs, m, axis=1).reshape(-1)
    j = np.tile(dofs, (1, m)).reshape(-1)
    v = (np.asarray(w)[:, None, None] * Ke).reshape(-1)
    keep = (i >= 0) & (j >= 0)
    return sp.coo_matrix((v[keep], (i[keep], j[keep])), shape=(n_free, n_free)).tocsr()


def element_energies(Ke, dofs, u):
    """ce[e] = u_e^T K_e u_e with Dirichlet dofs 0; ``u`` flat over the free dofs."""
    ue = np.where(dofs >= 0, np.asarray(u)[np.maximum(dofs, 0)], 0.0)
    return np.einsum("ei,eij,ej->e", ue, Ke, ue)


def geometry(coords, conn):
    """(centroids [ne, 2], volumes [ne]): corner mean and shoelace area."""
    X = np.asarray(coords, dtype=np.float64)[np.asarray(conn, dtype=np.int64)]
    Xn = np.roll(X, -1, axis=1)
    return X.mean(axis=1), 0.5 * np.abs((X[..., 0] * Xn[..., 1] - Xn[..., 0] * X[..., 1]).sum(axis=1))


def filter_matrix(centroids, volumes, radius):
    """Dense F [ne, ne] by brute force; ``radius <= 0``: the identity."""
    n = len(volumes)
    if radius <= 0:
        return np.eye(n)
    d = np.sqrt(((centroids[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2))
    H = np.maximum(0.0, radius - d) * np.asarray(volumes)[None, :]
    return H / H.sum(axis=1, keepdims=True)


def simp(rho_f, penal, e_min):
    return e_min + rho_f ** penal * (1.0 - e_min)


def oc_value(rho, dc, dv, lam, move):
    b = rho * np.sqrt(np.maximum(0.0, -dc / dv) / lam)
    return np.minimum(np.minimum(1.0, rho + move), np.maximum(np.maximum(0.0, rho - move), b))


def oc_bisect(rho, dc, dv, F, vol, vol_target, move, n_bisect):
    """The device's rule: bracket [0, R], R = max_e max(0, -dc_e / dv_e) (1 if that is 0); evaluate V at lambda_hi and, while it
    is infeasible, move the bracket up (lo = hi, hi x 4); then halve at m = (lo + hi) / 2 with V(m) <= vol_target moving hi,
    else lo; n_bisect + 1 evaluations in all; a midpoint equal to an end changes nothing.  Returns
    (rho_new at lambda_hi, lo, hi, feasible)."""
    V = lambda lam: float(vol @ (F @ oc_value(rho, dc, dv, lam, move)))
    R = float(np.maximum(0.0, -dc / dv).max())
    lo, hi, feasible, expand = 0.0, (R if R > 0 and np.isfinite(R) else 1.0), False, True
    for _ in range(n_bisect + 1):
        if expand:
            if V(hi) <= vol_target:
                feasible, expand = True, False
            elif np.isfinite(4.0 * hi):
                lo, hi = hi, 4.0 * hi
            continue
        m = 0.5 * (lo + hi)
        if not (lo < m < hi):
            continue
        if V(m) <= vol_target:
            hi = m
        else:
            lo = m
    return oc_value(rho, dc, dv, hi, move), lo, hi, feasible


def compliance_and_sensitivity(Ke, dofs, n_free, f, rho, F, penal, e_min, u=None):
    """(c, dc/drho, u, rho~) at design ``rho``: sparse direct solve unless ``u`` is given."""
    rf = F @ rho
    w = simp(rf, penal, e_min)
    if u is None:
        u = spla.spsolve(scaled_stiffness(Ke, dofs, w, n_free).tocsc(), f)
    ce = element_energies(Ke, dofs, u)
    c = float(w @ ce)
    dc = F.T @ (-penal * rf ** (penal - 1.0) * (1.0 - e_min) * ce)
    return c, dc, u, rf


def oc_loop(Ke, dofs, n_free, f, vol, F, volume_fraction, penal, e_min, move, n_bisect, n_iter):
    """The reference design loop from the uniform design.  Returns (compliances c_1..c_n, volumes after each update, feasible
    flags, final rho)."""
    rho = np.full(len(vol), float(volume_fraction))
    target = volume_fraction * float(vol.sum())
    dv = F.T @ vol
    cs, vs, fl = [], [], []
    for _ in range(n_iter):
        c, dc, _, _ = compliance_and_sensitivity(Ke, dofs, n_free, f, rho, F, penal, e_min)
        rho, lo, hi, ok = oc_bisect(rho, dc, dv, F, vol, target, move, n_bisect)
        cs.append(c)
        vs.append(float(vol @ (F @ rho)))
        fl.append(ok)
    return np.array(cs), np.array(vs), fl, rho


def edge_load(coords, edges, row_node_of, traction, ci=0.5, cj=0.5):
    """Nodal load of a constant traction vector on 2-node edges (i, j), flat over the free dofs (``row_node_of[n]`` = free row
    or -1): end i takes ``ci`` x traction x length and end j ``cj`` x that.  (1/2, 1/2) is the consistent load;
    ``EnergyLoss2D`` integrates with its own 1D rule, whose two sums it keeps as ``_ci`` and ``_cj``."""
    n_free = int((np.asarray(row_node_of) >= 0).sum())
    f = np.zeros(2 * n_free)
    for i, j in np.asarray(edges, dtype=np.int64):
        L = np.linalg.norm(coords[i] - coords[j])
        for n, c in ((i, ci), (j, cj)):
            r = row_node_of[n]
            if r >= 0:
                f[2 * r] += c * L * traction[0]
                f[2 * r + 1] += c * L * traction[1]
    return f
