"""tests/dynamics_reference.py pinned on a random SPD pencil of 12 dofs: the two exact properties of the average-acceleration
scheme (beta = 1/4, gamma = 1/2, C = 0) -- a single mode moves as phi cos(omega~ n dt) with tan(omega~ dt / 2) = omega dt / 2,
and the energy 1/2 v^T M v + 1/2 u^T K u - load u^T b is conserved under constant load -- and the sign of mass-proportional
damping.  CPU only."""
import numpy as np
import scipy.linalg

import dynamics_reference as DR

N = 12


def pencil(seed=0):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((N, N)), rng.standard_normal((N, N))
    K = a @ a.T + N * np.eye(N)
    M = b @ b.T + N * np.eye(N)
    w, V = scipy.linalg.eigh(K, M)                     # V^T M V = I
    return K, M, w, V, rng


def test_single_mode_closed_form():
    K, M, w, V, _ = pencil()
    for j in (0, 2, N - 1):
        phi, om = V[:, j], np.sqrt(w[j])
        dt = 2 * np.pi / om / 20
        U, Vv, A = DR.newmark(K, M, np.zeros(N), phi, np.zeros(N), dt, 40)
        omt = DR.discrete_frequency(om, dt)
        want = phi[None, :] * np.cos(omt * dt * np.arange(41))[:, None]
        err = np.abs(U - want).max()
        print(f"mode {j}: max |u - phi cos| = {err:.2e} (max |phi| {np.abs(phi).max():.2e})")
        assert err <= 1e-10 * np.abs(phi).max()
        assert np.abs(A[0] + w[j] * phi).max() <= 1e-10 * w[j] * np.abs(phi).max()      # M a0 = -K phi = -lambda M phi


def test_energy_is_conserved_under_constant_load():
    K, M, w, V, rng = pencil(1)
    b = rng.standard_normal(N)
    dt = 2 * np.pi / np.sqrt(w[0]) / 20
    U, Vv, A = DR.newmark(K, M, b, np.zeros(N), np.zeros(N), dt, 40)
    E = np.array([DR.energy(K, M, b, u, v) for u, v in zip(U, Vv)])
    drift, peak = np.ptp(E[:, 3]), E[:, 0].max()
    print(f"energy drift {drift:.2e}, peak kinetic {peak:.2e}")
    assert peak > 0 and drift <= 1e-12 * peak
    # not conserved off the average-acceleration parameters: the check above can fail
    U2, V2, _ = DR.newmark(K, M, b, np.zeros(N), np.zeros(N), dt, 40, beta=0.3025, gamma=0.6)
    E2 = np.array([DR.energy(K, M, b, u, v)[3] for u, v in zip(U2, V2)])
    assert np.ptp(E2) > 1e-6 * peak


def test_mass_proportional_damping_shrinks_a_single_mode_every_period():
    K, M, w, V, _ = pencil(2)
    phi, om = V[:, 1], np.sqrt(w[1])
    dt, per = 2 * np.pi / om / 20, 20
    alpha = 0.1 * om
    n = 6 * per
    U, _, _ = DR.newmark(K, M, np.zeros(N), phi, np.zeros(N), dt, n, alpha_r=alpha)
    U0, _, _ = DR.newmark(K, M, np.zeros(N), phi, np.zeros(N), dt, n)
    q, q0 = U @ (M @ phi), U0 @ (M @ phi)             # modal coordinates (phi^T M phi = 1)
    assert np.abs(U - q[:, None] * phi[None, :]).max() <= 1e-10 * np.abs(phi).max()     # C = alpha M keeps the mode
    amp = np.array([np.abs(q[k * per:(k + 1) * per + 1]).max() for k in range(6)])
    amp0 = np.array([np.abs(q0[k * per:(k + 1) * per + 1]).max() for k in range(6)])
    print("damped peaks per period", amp, "undamped", amp0)
    assert (amp <= amp0 + 1e-12).all() and (amp[1:] < amp0[1:]).all()
    assert (np.diff(amp) < 0).all()
    # the continuous envelope exp(-alpha t / 2) within the scheme's period error
    assert abs(amp[3] / amp[2] - np.exp(-0.5 * alpha * per * dt)) <= 0.05


def test_step_equals_the_trajectory_and_stiffness_damping_enters_through_w():
    K, M, w, V, rng = pencil(3)
    b = rng.standard_normal(N)
    dt = 0.05
    load = lambda t: np.sin(3.0 * t)
    kw = dict(beta=0.25, gamma=0.5, alpha_r=0.3, beta_r=0.02)
    U, Vv, A = DR.newmark(K, M, b, rng.standard_normal(N), rng.standard_normal(N), dt, 5, load=load, **kw)
    C = kw["alpha_r"] * M + kw["beta_r"] * K
    for k in range(6):                                   # the equation of motion holds at every step
        r = M @ A[k] + C @ Vv[k] + K @ U[k] - load(k * dt) * b
        assert np.abs(r).max() <= 1e-10 * np.abs(K @ U[k]).max()
    u, v, a = DR.step(K, M, b, U[2], Vv[2], A[2], dt, load(3 * dt), **kw)
    assert np.array_equal(u, U[3]) and np.array_equal(v, Vv[3]) and np.array_equal(a, A[3])
