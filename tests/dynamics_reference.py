"""Dense numpy statement of Newmark time stepping in the a-form, shared by the dynamics tests (a plain helper
module, not a conftest): direct solves, no iteration, independent of the kernels.

    M u'' + C u' + K u = load(t) b,   C = alpha_R M + beta_R K
    u~ = u + dt v + dt^2 (1/2 - beta) a     v~ = v + dt (1 - gamma) a     w = u~ + beta_R v~
    A a+ = load(t + dt) b - K w - alpha_R M v~,   A = c_M M + c_K K,  c_M = 1 + gamma dt alpha_R,  c_K = beta dt^2 + gamma dt beta_R
    u+ = u~ + beta dt^2 a+                  v+ = v~ + gamma dt a+
    M a0 = load(0) b - K u0 - C v0

The mass matrix of a mesh comes from tests/modal_reference.py.
"""
import numpy as np
import scipy.linalg


def coefficients(dt, beta=0.25, gamma=0.5, alpha_r=0.0, beta_r=0.0):
    """(c_K, c_M) of the step operator A = c_M M + c_K K."""
    return beta * dt * dt + gamma * dt * beta_r, 1.0 + gamma * dt * alpha_r


def initial_acceleration(K, M, b, u0, v0, alpha_r=0.0, beta_r=0.0, load0=1.0):
    return np.linalg.solve(M, load0 * b - K @ (u0 + beta_r * v0) - alpha_r * (M @ v0))


def step(K, M, b, u, v, a, dt, load1, beta=0.25, gamma=0.5, alpha_r=0.0, beta_r=0.0, factor=None):
    """One step from (u, v, a) to (u+, v+, a+); ``factor``: ``scipy.linalg.cho_factor`` of A (formed when None)."""
    c_k, c_m = coefficients(dt, beta, gamma, alpha_r, beta_r)
    if factor is None:
        factor = scipy.linalg.cho_factor(c_m * M + c_k * K)
    ut = u + dt * v + dt * dt * (0.5 - beta) * a
    vt = v + dt * (1.0 - gamma) * a
    w = ut + beta_r * vt
    a1 = scipy.linalg.cho_solve(factor, load1 * b - K @ w - alpha_r * (M @ vt))
    return ut + beta * dt * dt * a1, vt + gamma * dt * a1, a1


def newmark(K, M, b, u0, v0, dt, n, beta=0.25, gamma=0.5, alpha_r=0.0, beta_r=0.0, load=None):
    """The trajectory (U, V, A), each [n + 1, ndof]; row 0 is the initial state with the solved a0."""
    load = (lambda t: 1.0) if load is None else load
    c_k, c_m = coefficients(dt, beta, gamma, alpha_r, beta_r)
    factor = scipy.linalg.cho_factor(c_m * M + c_k * K)
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    a = initial_acceleration(K, M, b, u, v, alpha_r, beta_r, load(0.0))
    U, V, A = [u], [v], [a]
    for k in range(n):
        u, v, a = step(K, M, b, u, v, a, dt, load((k + 1) * dt), beta, gamma, alpha_r, beta_r, factor)
        U.append(u); V.append(v); A.append(a)
    return np.array(U), np.array(V), np.array(A)


def energy(K, M, b, u, v, load=1.0):
    """(kinetic, strain, work, total) = (1/2 v^T M v, 1/2 u^T K u, load u^T b, kinetic + strain - work)."""
    kin, strain, work = 0.5 * v @ (M @ v), 0.5 * u @ (K @ u), load * (u @ b)
    return kin, strain, work, kin + strain - work


def discrete_frequency(omega, dt):
    """The frequency the average-acceleration scheme (beta = 1/4, gamma = 1/2, no damping) moves a mode of frequency omega
    with: u_n = phi cos(omega~ n dt), tan(omega~ dt / 2) = omega dt / 2."""
    return 2.0 / dt * np.arctan(0.5 * omega * dt)
