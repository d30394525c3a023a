"""Numpy fp64 statement of small-strain J2 elastoplasticity on TRI3 meshes in plane strain, shared by the tests (a
plain helper module, not a conftest).  It imports nothing from the library's compute paths.

Physical gradient convention; one state point per element; element area A_e = |det J| W with W the sum of the triangle Gauss
weights.  mu = E / (2 (1 + nu)), lambda = E nu / ((1 + nu)(1 - 2 nu)), kappa = lambda + 2 mu / 3.  Committed state per element:
eps^p = (xx, yy, xy) in tensor components (zz = -xx - yy) and alpha.  For a total strain eps with eps_zz = 0:

    tr = eps_xx + eps_yy,   s_tr = 2 mu (dev eps - eps^p_n)           (xx, yy, zz, xy; dev eps_zz = -tr / 3)
    |s_tr| = sqrt(s_xx^2 + s_yy^2 + s_zz^2 + 2 s_xy^2),   f = |s_tr| - sqrt(2/3) (sigma_y + H alpha_n),   D = 2 mu + 2 H / 3
    f <= 0: dgamma = 0;   f > 0: dgamma = f / D;   n = s_tr / |s_tr|
    eps^p = eps^p_n + dgamma n,  alpha = alpha_n + sqrt(2/3) dgamma,  s = s_tr - 2 mu dgamma n,  sigma = kappa tr I + s
    Psi = kappa tr^2 / 2 + |s_tr|^2 / (4 mu) - <f>^2 / (2 D)
    theta = 1 - 2 mu dgamma / |s_tr|,   theta_bar = 1 / (1 + H / (3 mu)) - (1 - theta)       (elastic: 1 and 0)
    dsigma = kappa tr(deps) I + 2 mu theta dev(deps) - 2 mu theta_bar (n : deps) n

The driver is the algorithm of ``hidenn_fem_amd.plasticity.ElastoplasticSolver`` (``tests/newton_reference.py``'s, in numpy) on
dense matrices: block-Jacobi PCG truncated on p^T K p <= 0, Eisenstat-Walker choice 2, backtracking on
Pi(u + t d) <= Pi(u) + armijo t g.d + 4 eps |Pi(u)|.
"""
from dataclasses import dataclass, field as _field

import numpy as np

EPS = 2.2e-16
RT23 = np.sqrt(2.0 / 3.0)
WV = np.array([1.0, 1.0, 2.0])      # sigma : eps = s_xx e_xx + s_yy e_yy + 2 s_xy e_xy


@dataclass
class Material:
    E: float = 10e9
    nu: float = 0.3
    sigma_y: float = 1e5
    H: float = 5e8

    @property
    def mu(self):
        return self.E / (2 * (1 + self.nu))

    @property
    def lam(self):
        return self.E * self.nu / ((1 + self.nu) * (1 - 2 * self.nu))

    @property
    def kappa(self):
        return self.lam + 2 * self.mu / 3


# ---------------------------------------------------------------- the constitutive law, vectorised over points
def return_map(eps, ep, al, mat):
    """eps, ep [n, 3] = (xx, yy, xy), al [n] -> dict(psi, sig [n, 4] = (xx, yy, xy, zz), ep, al, plastic, dgamma, theta,
    theta_bar, n [n, 4] = (xx, yy, zz, xy), f, nrm)."""
    mu, kap, sy, H = mat.mu, mat.kappa, mat.sigma_y, mat.H
    tr = eps[:, 0] + eps[:, 1]
    d = np.stack([eps[:, 0] - tr / 3, eps[:, 1] - tr / 3, -tr / 3, eps[:, 2]], 1)
    s = 2 * mu * (d - np.stack([ep[:, 0], ep[:, 1], -(ep[:, 0] + ep[:, 1]), ep[:, 2]], 1))
    nrm = np.sqrt(s[:, 0] ** 2 + s[:, 1] ** 2 + s[:, 2] ** 2 + 2 * s[:, 3] ** 2)
    f = nrm - RT23 * (sy + H * al)
    pl = f > 0
    D = 2 * mu + 2 * H / 3
    dg = np.where(pl, f / D, 0.0)
    safe = np.where(nrm > 0, nrm, 1.0)
    n = s / safe[:, None]
    psi = 0.5 * kap * tr ** 2 + nrm ** 2 / (4 * mu) - np.where(pl, f * f / (2 * D), 0.0)
    sn = s - 2 * mu * dg[:, None] * n
    sig = np.stack([kap * tr + sn[:, 0], kap * tr + sn[:, 1], sn[:, 3], kap * tr + sn[:, 2]], 1)
    theta = np.where(pl, 1 - 2 * mu * dg / safe, 1.0)
    theta_bar = np.where(pl, 1 / (1 + H / (3 * mu)) - (1 - theta), 0.0)
    return dict(psi=psi, sig=sig, ep=ep + dg[:, None] * n[:, [0, 1, 3]], al=al + RT23 * dg, plastic=pl, dgamma=dg, theta=theta,
                theta_bar=theta_bar, n=n, f=f, nrm=nrm)


def tangent_moduli(r, mat):
    """-> C [n, 3, 3]: d(s_xx, s_yy, s_xy) / d(e_xx, e_yy, e_xy) (tensor shear component)."""
    mu, kap = mat.mu, mat.kappa
    idev = np.array([[2 / 3, -1 / 3, 0], [-1 / 3, 2 / 3, 0], [0, 0, 1.0]])
    vol = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0.0]])
    n = r["n"]
    nn = np.stack([n[:, 0], n[:, 1], n[:, 3]], 1)
    nw = np.stack([n[:, 0], n[:, 1], 2 * n[:, 3]], 1)
    return kap * vol[None] + 2 * mu * r["theta"][:, None, None] * idev[None] \
        - 2 * mu * r["theta_bar"][:, None, None] * nn[:, :, None] * nw[:, None, :]


def von_mises(sig):
    p = (sig[:, 0] + sig[:, 1] + sig[:, 3]) / 3
    return np.sqrt(1.5 * ((sig[:, 0] - p) ** 2 + (sig[:, 1] - p) ** 2 + (sig[:, 3] - p) ** 2 + 2 * sig[:, 2] ** 2))


# ---------------------------------------------------------------- the mesh: B, areas, assembly
class Mesh:
    def __init__(self, coords, conn, W=0.5):
        self.X = np.asarray(coords, dtype=np.float64)
        self.T = np.asarray(conn, dtype=np.int64)
        self.ne, self.nn = self.T.shape[0], self.X.shape[0]
        Xe = self.X[self.T]
        Jg = np.stack([Xe[:, 0] - Xe[:, 2], Xe[:, 1] - Xe[:, 2]], axis=2)
        det = Jg[:, 0, 0] * Jg[:, 1, 1] - Jg[:, 0, 1] * Jg[:, 1, 0]
        dN = np.einsum("kj,eji->eki", np.array([[1, 0], [0, 1], [-1, -1]], float), np.linalg.inv(Jg))   # dN_k / dx_i
        self.A = np.abs(det) * W
        B = np.zeros((self.ne, 3, 6))
        for k in range(3):
            B[:, 0, 2 * k] = dN[:, k, 0]
            B[:, 1, 2 * k + 1] = dN[:, k, 1]
            B[:, 2, 2 * k] = 0.5 * dN[:, k, 1]
            B[:, 2, 2 * k + 1] = 0.5 * dN[:, k, 0]
        self.B = B
        self.dofs = (2 * self.T[:, :, None] + np.arange(2)[None, None, :]).reshape(self.ne, 6)

    def strain(self, u):
        return np.einsum("esd,ed->es", self.B, u[self.T].reshape(self.ne, 6))

    def f_int(self, sig):
        fe = self.A[:, None] * np.einsum("es,esd->ed", sig[:, :3] * WV, self.B)
        f = np.zeros(2 * self.nn)
        np.add.at(f, self.dofs.ravel(), fe.ravel())
        return f.reshape(-1, 2)

    def K(self, C):
        Ke = self.A[:, None, None] * np.einsum("esd,s,est,etf->edf", self.B, WV, C, self.B)
        K = np.zeros((2 * self.nn, 2 * self.nn))
        np.add.at(K, (self.dofs[:, :, None].repeat(6, 2).ravel(), self.dofs[:, None, :].repeat(6, 1).ravel()), Ke.ravel())
        return K


# The engine tabulates edge loads as EnergyLoss2D does (and as the project it was modelled on does): T_i = sum_q w_q (1 - xi_q) t,
# T_j = sum_q w_q xi_q t with the RAW two-point Legendre rule on [-1, 1] (w = 1, 1; xi = -+1/sqrt 3), times the edge length.  For
# a constant traction that is c_i = 2, c_j = 0: the first node of every edge receives 2 L t.  A traction callable t therefore
# loads an edge with the resultant 2 L t.
EDGE_C = (2.0, 0.0)


def edge_loads(coords, edges, traction):
    """f_ext [Nn, 2] of a CONSTANT traction callable value (tx, ty) on two-node edges, as the engine tabulates it."""
    X = np.asarray(coords, dtype=np.float64)
    f = np.zeros_like(X)
    for a, b in np.asarray(edges):
        L = np.linalg.norm(X[a] - X[b])
        f[a] += EDGE_C[0] * L * np.asarray(traction)
        f[b] += EDGE_C[1] * L * np.asarray(traction)
    return f


class Problem:
    """A mesh, a material, Dirichlet rows ``bc`` (bool [Nn]; values ``u_fixed`` [n_fixed, 2] at load 1) and nodal loads
    ``f_ext`` [Nn, 2] at load 1.  Unknowns: the free rows in node order.  The committed state is an argument everywhere."""

    def __init__(self, coords, conn, bc, mat, W=0.5, u_fixed=None, f_ext=None):
        self.mesh, self.mat = Mesh(coords, conn, W), mat
        self.bc = np.asarray(bc, dtype=bool)
        self.free = ~self.bc
        self.n = int(self.free.sum())
        self.u_fixed = np.zeros((int(self.bc.sum()), 2)) if u_fixed is None else np.asarray(u_fixed, dtype=np.float64)
        self.f_ext = np.zeros((self.mesh.nn, 2)) if f_ext is None else np.asarray(f_ext, dtype=np.float64)
        self.fdof = np.nonzero(np.repeat(self.free, 2))[0]

    def virgin(self):
        return np.zeros((self.mesh.ne, 3)), np.zeros(self.mesh.ne)

    def full(self, uf, load):
        u = np.zeros((self.mesh.nn, 2))
        u[self.free] = uf
        u[self.bc] = load * self.u_fixed
        return u

    def point(self, uf, ep, al, load):
        return return_map(self.mesh.strain(self.full(uf, load)), ep, al, self.mat)

    def energy(self, uf, ep, al, load):
        """-> (Pi, g [n, 2], return-map dict)"""
        r = self.point(uf, ep, al, load)
        fx = load * self.f_ext[self.free]
        g = self.mesh.f_int(r["sig"])[self.free] - fx
        return float((self.mesh.A * r["psi"]).sum() - (fx * uf).sum()), g, r

    def tangent(self, uf, ep, al, load, full=False):
        K = self.mesh.K(tangent_moduli(self.point(uf, ep, al, load), self.mat))
        return K if full else K[np.ix_(self.fdof, self.fdof)]


# ---------------------------------------------------------------- block-Jacobi PCG and the Newton step (the device's)
def diag_blocks(Kff):
    i = 2 * np.arange(Kff.shape[0] // 2)
    return np.stack([Kff[i, i], 0.5 * (Kff[i, i + 1] + Kff[i + 1, i]), Kff[i + 1, i + 1]], 1)


def jacobi_inverse(b):
    det = b[:, 0] * b[:, 2] - b[:, 1] ** 2
    pd = (det > 0) & (b[:, 0] > 0) & np.isfinite(det)
    s = np.where(pd, det, 1.0)
    return np.stack([np.where(pd, b[:, 2] / s, 1.0), np.where(pd, -b[:, 1] / s, 0.0), np.where(pd, b[:, 0] / s, 1.0)], 1)


def apply_blocks(dinv, r):
    return np.stack([dinv[:, 0] * r[:, 0] + dinv[:, 1] * r[:, 1], dinv[:, 1] * r[:, 0] + dinv[:, 2] * r[:, 1]], 1)


def pcg(K, dinv, g, eta, max_iter):
    n = g.shape[0]
    d, r = np.zeros_like(g), -g.copy()
    z = apply_blocks(dinv, r)
    rho, tol, p, beta, it = (r * z).sum(), eta * np.linalg.norm(g), np.zeros_like(g), 0.0, 0
    if np.linalg.norm(r) <= tol:
        return d, 0, "rtol"
    while True:
        p = z + beta * p
        q = (K @ p.reshape(-1)).reshape(n, 2)
        pq = (p * q).sum()
        if not pq > 0 or not np.isfinite(rho / pq):
            return d, it, "breakdown"
        alpha = rho / pq
        d, r = d + alpha * p, r - alpha * q
        z = apply_blocks(dinv, r)
        rho_new = (r * z).sum()
        beta, rho = rho_new / rho, rho_new
        it += 1
        if np.linalg.norm(r) <= tol:
            return d, it, "rtol"
        if it >= max_iter:
            return d, it, "max_iter"


@dataclass
class Result:
    u: np.ndarray
    ep: np.ndarray = None
    al: np.ndarray = None
    sig: np.ndarray = None
    plastic: np.ndarray = None
    newton_iterations: int = 0
    cg_iterations: int = 0
    grad_norm: float = 0.0
    rhs_norm: float = 0.0
    energy: float = 0.0
    converged: bool = False
    reason: str = ""
    history: list = _field(default_factory=list)


def step(prob, u0, ep, al, load, rtol=1e-10, atol=0.0, max_newton=50, eta_max=0.1, armijo=1e-4, max_backtracks=30, exact=False):
    """One load step from the free rows ``u0`` against the committed state (ep, al).  ``exact``: solve every Newton system
    directly instead of by truncated PCG (the line search stays).  The result carries the TRIAL state of its ``u``."""
    u = u0.copy()
    rhs = np.linalg.norm(prob.energy(np.zeros_like(u), ep, al, load)[1])
    tol = max(rtol * rhs, atol)
    E, g, r = prob.energy(u, ep, al, load)
    res = Result(u=u, rhs_norm=rhs)
    gn_prev, k = None, 0
    while True:
        gn = np.linalg.norm(g)
        res.grad_norm, res.energy, res.newton_iterations = gn, E, k
        if gn <= tol:
            res.converged, res.reason = True, "rtol" if rtol * rhs >= atol else "atol"
            break
        if k >= max_newton:
            res.reason = "max_newton"
            break
        eta = eta_max if gn_prev is None else min(max(0.9 * (gn / gn_prev) ** 2, 1e-12), eta_max)
        K = prob.tangent(u, ep, al, load)
        if exact:
            d, its, halt = -np.linalg.solve(K, g.reshape(-1)).reshape(-1, 2), 0, "rtol"
        else:
            dinv = jacobi_inverse(diag_blocks(K))
            d, its, halt = pcg(K, dinv, g, eta, max(1000, 4 * prob.n))
            if halt == "breakdown" and its == 0:
                d = -apply_blocks(dinv, g)
        res.cg_iterations += its
        gtd = (g * d).sum()
        t, ok = 1.0, False
        for _ in range(max_backtracks + 1):
            Et, gt, rt = prob.energy(u + t * d, ep, al, load)
            if np.isfinite(Et) and Et <= E + armijo * t * gtd + 4 * EPS * abs(E):
                ok = True
                break
            t *= 0.5
        res.history.append(dict(energy=E, grad_norm=gn, eta=eta, cg_iterations=its, cg_reason=halt, step=t if ok else 0.0))
        if not ok:
            res.reason = "line_search"
            break
        u, gn_prev, E, g, r = u + t * d, gn, Et, gt, rt
        k += 1
    res.u, res.ep, res.al, res.sig, res.plastic = u, r["ep"], r["al"], r["sig"], r["plastic"]
    return res


def path(prob, loads, **kw):
    """The load path from the virgin state and u = 0: every step starts from the last equilibrium and commits.  -> [Result]"""
    ep, al = prob.virgin()
    u = np.zeros((prob.n, 2))
    out = []
    for load in loads:
        res = step(prob, u, ep, al, load, **kw)
        u, ep, al = res.u, res.ep, res.al
        out.append(res)
    return out


# ---------------------------------------------------------------- the two cantilever paths of the GPU tests
LOADS = [0.25, 0.5, 0.75, 1.0, 0.6, 0.2, -0.2, -0.6]
CANTILEVERS = {"23x17": (23, 17, 6e4), "17x9": (17, 9, 1e5)}      # nx, ny, sigma_y
# A vertical traction of 2e4 on the right edge: resultant 2e4 per unit length.  The engine's edge rule weighs a callable's
# value by 2 (EDGE_C), so the callable handed to the solver -- and to edge_loads -- is (0, 1e4).
TRACTION = (0.0, 1e4)
_cant = {}


def cantilever(name):
    """-> (mesh tuple of structured_tri_mesh on [0, 2] x [0, 1], Problem): left edge clamped, vertical traction 2e4 on the
    right edge, E = 10e9, nu = 0.3, H = 5e8."""
    if name not in _cant:
        import torch
        from hidenn_fem_amd.mesh import structured_tri_mesh
        nx, ny, sy = CANTILEVERS[name]
        ms = structured_tri_mesh(nx, ny, dtype=torch.float64)
        coords, conn, _, bc, _, edges = ms
        prob = Problem(coords.numpy(), conn.numpy(), bc.numpy(), Material(sigma_y=sy), 0.5, None,
                       edge_loads(coords.numpy(), edges.numpy(), TRACTION))
        _cant[name] = (ms, prob)
    return _cant[name]


_paths = {}


def cantilever_path(name):
    if name not in _paths:
        _paths[name] = path(cantilever(name)[1], LOADS, rtol=1e-10)
    return _paths[name]
