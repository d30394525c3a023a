"""Dense numpy statement of Newmark time stepping at finite strain, shared by the finite-strain dynamics tests (a
plain helper module, not a conftest): dense tangents, direct solves, full Newton, independent of the kernels.

    M u'' + alpha_R M u' + f_int(u) = load(t) b
    u~ = u + dt v + dt^2 (1/2 - beta) a      v~ = v + dt (1 - gamma) a
    R(a+) = c_M M a+ + alpha_R M v~ + f_int(u~ + c_K a+) - load(t + dt) b = 0,   c_K = beta dt^2,  c_M = 1 + gamma dt alpha_R
    J(a+) = dR/da+ = c_M M + c_K K_T(u~ + c_K a+)
    Phi(a+) = Pi_int(u~ + c_K a+) - load b . (u~ + c_K a+) + c_K [1/2 c_M a+^T M a+ + alpha_R a+^T M v~],   grad Phi = c_K R
    u+ = u~ + beta dt^2 a+                   v+ = v~ + gamma dt a+
    M a0 = load(0) b - f_int(u0) - alpha_R M v0

``System`` holds one mesh: the internal energy, its gradient and its tangent come from the dense statements of the Neo-Hookean
element the static tests use (``newton_reference.Problem`` / ``quad4_newton_reference.Problem`` WITHOUT edge loads), the mass from
``modal_reference.mass``.  Vectors are flat numpy arrays [2 n] over the free rows in node order, interleaved (x, y).
"""
import numpy as np
import scipy.linalg
import torch

import modal_reference as MR

F64 = torch.float64


def coefficients(dt, beta=0.25, gamma=0.5, alpha_r=0.0):
    """(c_K, c_M) of the step operator A = c_M M + c_K K_T."""
    return beta * dt * dt, 1.0 + gamma * dt * alpha_r


class System:
    """``prob``: a ``Problem`` of ``newton_reference`` or ``quad4_newton_reference`` built with ``edges=None`` (its energy is
    Pi_int alone); ``b`` [2 n]: the external load vector; ``rho``, ``lumped``: the mass."""

    def __init__(self, prob, b, rho=1.0, lumped=False):
        self.prob, self.n = prob, prob.n
        self.b = np.asarray(b, dtype=np.float64).reshape(-1)
        nodes = np.nonzero(prob.free.numpy())[0]
        self.M = MR.free_rows(MR.mass(prob.coords.numpy(), prob.conn.numpy(), rho=rho, lumped=lumped), nodes)
        self.lumped = lumped

    def _rows(self, u):
        return torch.as_tensor(np.asarray(u, dtype=np.float64).reshape(self.n, 2))

    def energy(self, u):
        """-> (Pi_int, f_int [2 n], min J, inverted count)"""
        e, g, mj, cnt = self.prob.energy(self._rows(u))
        return float(e), g.numpy().reshape(-1).copy(), float(mj), int(cnt)

    def f_int(self, u):
        return self.energy(u)[1]

    def K_T(self, u):
        K = self.prob.tangent(self._rows(u)).numpy()
        return 0.5 * (K + K.T)


def external_load(prob_loaded):
    """b = f_int(0) - g(0) of a ``Problem`` WITH its edge loads: the dead loads, as the solver forms them."""
    zero = torch.zeros(prob_loaded.n, 2, dtype=F64)
    full = prob_loaded.energy(zero)[1]
    edges, T = prob_loaded.edges, prob_loaded.T
    prob_loaded.edges, prob_loaded.T = None, None
    try:
        internal = prob_loaded.energy(zero)[1]
    finally:
        prob_loaded.edges, prob_loaded.T = edges, T
    return (internal - full).numpy().reshape(-1).copy()


def predictor(u, v, a, dt, beta=0.25, gamma=0.5):
    return u + dt * v + dt * dt * (0.5 - beta) * a, v + dt * (1.0 - gamma) * a


def residual(sys, a1, ut, vt, dt, load1, beta=0.25, gamma=0.5, alpha_r=0.0):
    c_k, c_m = coefficients(dt, beta, gamma, alpha_r)
    return c_m * (sys.M @ a1) + alpha_r * (sys.M @ vt) + sys.f_int(ut + c_k * a1) - load1 * sys.b


def jacobian(sys, a1, ut, dt, beta=0.25, gamma=0.5, alpha_r=0.0):
    c_k, c_m = coefficients(dt, beta, gamma, alpha_r)
    return c_m * sys.M + c_k * sys.K_T(ut + c_k * a1)


def potential(sys, a1, ut, vt, dt, load1, beta=0.25, gamma=0.5, alpha_r=0.0):
    c_k, c_m = coefficients(dt, beta, gamma, alpha_r)
    u1 = ut + c_k * a1
    return sys.energy(u1)[0] - load1 * (sys.b @ u1) + c_k * (0.5 * c_m * (a1 @ (sys.M @ a1)) + alpha_r * (a1 @ (sys.M @ vt)))


def initial_acceleration(sys, u0, v0, alpha_r=0.0, load0=1.0):
    return np.linalg.solve(sys.M, load0 * sys.b - sys.f_int(u0) - alpha_r * (sys.M @ v0))


def _phi(sys, a1, ut, vt, dt, load1, beta, gamma, alpha_r):
    """-> (Phi, the sum of the magnitudes of its terms, inverted count) at a1"""
    c_k, c_m = coefficients(dt, beta, gamma, alpha_r)
    u1 = ut + c_k * a1
    pi, _, _, cnt = sys.energy(u1)
    work, inertia, damping = load1 * (sys.b @ u1), c_k * 0.5 * c_m * (a1 @ (sys.M @ a1)), c_k * alpha_r * (a1 @ (sys.M @ vt))
    return pi - work + inertia + damping, abs(pi) + abs(work) + abs(inertia) + abs(damping), cnt


def _descent_direction(J, M, R):
    """d = -(J + tau M)^-1 R with the smallest tau in {0, 1e-3 |J| / |M| x 4^k} that makes J + tau M positive definite
    (Cholesky succeeds): the Newton direction where J is, a descent direction of Phi always."""
    tau, unit = 0.0, 1e-3 * np.abs(J).max() / np.abs(M).max()
    while True:
        try:
            c = scipy.linalg.cho_factor(J + tau * M)
            return -scipy.linalg.cho_solve(c, R)
        except np.linalg.LinAlgError:
            tau = unit if tau == 0.0 else 4.0 * tau


def step(sys, u, v, a, dt, load1, beta=0.25, gamma=0.5, alpha_r=0.0, rtol=1e-13, max_newton=60):
    """One step from (u, v, a) by Newton with dense solves as a MINIMISATION of the incremental potential Phi, as the device
    does it: started at the previous a (at u+ = u where that start has an inverted element); the direction is Newton's where the
    Jacobian is positive definite and that of the Jacobian shifted by a multiple of M where it is not; the full step is halved
    while the trial state has an inverted element or Phi fails the Armijo test (1e-4; rounding slack 4 eps times the
    magnitudes of Phi's terms).  Ends at ||R|| <= rtol ||R(a = 0)||, or where ||R|| stops falling below 1e-6 ||R(a = 0)||: the
    rounding floor.  -> (u+, v+, a+, ||R|| at a+, min J at u+)"""
    c_k, _ = coefficients(dt, beta, gamma, alpha_r)
    ut, vt = predictor(u, v, a, dt, beta, gamma)
    kw = dict(beta=beta, gamma=gamma, alpha_r=alpha_r)
    r0 = np.linalg.norm(residual(sys, np.zeros_like(a), ut, vt, dt, load1, **kw))
    a1 = np.array(a, dtype=np.float64)
    if c_k > 0.0 and sys.energy(ut + c_k * a1)[3] > 0:      # the extrapolated start is inverted: start at u+ = u instead
        a1 = (u - ut) / c_k
    R = residual(sys, a1, ut, vt, dt, load1, **kw)
    rn = np.linalg.norm(R)
    phi, mag, _ = _phi(sys, a1, ut, vt, dt, load1, beta, gamma, alpha_r)
    for _ in range(max_newton):
        if rn <= rtol * r0:
            break
        d = _descent_direction(jacobian(sys, a1, ut, dt, **kw), sys.M, R)
        slope = c_k * (R @ d)
        s, found = 1.0, False
        for _ in range(30):
            trial = a1 + s * d
            phi_t, mag_t, cnt = _phi(sys, trial, ut, vt, dt, load1, beta, gamma, alpha_r)
            if cnt == 0 and phi_t <= phi + 1e-4 * s * slope + 4 * 2.2e-16 * mag:
                found = True
                break
            s *= 0.5
        if not found:
            break
        Rt = residual(sys, trial, ut, vt, dt, load1, **kw)
        rt = np.linalg.norm(Rt)
        if not rt < rn and rn <= 1e-6 * r0:                 # the rounding floor: keep the better iterate
            break
        a1, R, rn, phi, mag = trial, Rt, rt, phi_t, mag_t
    u1 = ut + c_k * a1
    return u1, vt + gamma * dt * a1, a1, rn, sys.energy(u1)[2]


def explicit_step(sys, u, v, a, dt, load1, gamma=0.5, alpha_r=0.0):
    """Central difference (beta = 0) with a lumped mass: u+ = u~ is known, a+ = D^-1 rhs with D = c_M M diagonal.
    -> (u+, v+, a+, rhs)"""
    assert sys.lumped
    ut, vt = predictor(u, v, a, dt, 0.0, gamma)
    c_m = 1.0 + gamma * dt * alpha_r
    rhs = load1 * sys.b - sys.f_int(ut) - alpha_r * (sys.M @ vt)
    a1 = rhs / (c_m * np.diag(sys.M))
    return ut, vt + gamma * dt * a1, a1, rhs


def energy(sys, u, v, load=1.0):
    """(kinetic, strain, work, total) = (1/2 v^T M v, Pi_int(u), load b . u, kinetic + strain - work)."""
    kin, strain, work = 0.5 * v @ (sys.M @ v), sys.energy(u)[0], load * (sys.b @ u)
    return kin, strain, work, kin + strain - work


def trajectory(sys, u0, v0, dt, n, load=None, **kw):
    """(U, V, A) [n + 1, 2 n], the per-step ||R|| and min J; row 0 carries the solved a0."""
    load = (lambda t: 1.0) if load is None else load
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    a = initial_acceleration(sys, u, v, kw.get("alpha_r", 0.0), load(0.0))
    U, V, A, Rn, Jm = [u], [v], [a], [], []
    for k in range(n):
        u, v, a, rn, mj = step(sys, u, v, a, dt, load((k + 1) * dt), **kw)
        U.append(u); V.append(v); A.append(a); Rn.append(rn); Jm.append(mj)
    return np.array(U), np.array(V), np.array(A), np.array(Rn), np.array(Jm)
