"""The numpy statement of J2 elastoplasticity (tests/plasticity_reference.py) pinned on its own: finite differences, the
structure of the tangent, the elastic limit, the exactness of the radial return on proportional paths, and conditions on the two
cantilever load paths the GPU tests use -- so that no GPU test is vacuous."""
import numpy as np
import pytest

import plasticity_reference as P


def random_points(n=400, seed=0):
    rng = np.random.default_rng(seed)
    # the yield strain is sqrt(2/3) sigma_y / (2 mu) ~ 1e-5 for sigma_y = 1e5
    return rng.normal(size=(n, 3)) * 8e-6, rng.normal(size=(n, 3)) * 2e-6, np.abs(rng.normal(size=n)) * 5e-5


@pytest.mark.parametrize("H", [5e8, 0.0], ids=["hardening", "perfect"])
def test_central_differences_of_the_potential_and_of_the_stress(H):
    mat = P.Material(sigma_y=1e5, H=H)
    eps, ep, al = random_points()
    r = P.return_map(eps, ep, al, mat)
    frac = r["plastic"].mean()
    assert 0.2 <= frac <= 0.8, frac                                      # both branches present
    C = P.tangent_moduli(r, mat)
    h = 1e-9
    e_sig = e_C = 0.0
    away = np.abs(r["f"]) > 1e-3 * r["nrm"]                              # a difference must not straddle the yield surface
    assert away.mean() > 0.9
    for j in range(3):
        d = np.zeros(3)
        d[j] = h
        rp, rm = P.return_map(eps + d, ep, al, mat), P.return_map(eps - d, ep, al, mat)
        g = (rp["psi"] - rm["psi"]) / (2 * h)
        e_sig = max(e_sig, np.abs(g - r["sig"][:, j] * P.WV[j])[away].max() / np.abs(r["sig"]).max())
        dC = (rp["sig"][:, :3] - rm["sig"][:, :3]) / (2 * h)
        e_C = max(e_C, np.abs(dC - C[:, :, j])[away].max() / np.abs(C).max())
    print("H", H, "plastic", frac, "dPsi vs sigma", e_sig, "dsigma vs C", e_C)
    assert e_sig <= 1e-6 and e_C <= 1e-6


def small_problem(sigma_y=1e5, H=5e8):
    import torch
    from hidenn_fem_amd.mesh import structured_tri_mesh
    coords, conn, _, bc, _, edges = structured_tri_mesh(7, 5, jitter=0.2, seed=3, dtype=torch.float64)
    prob = P.Problem(coords.numpy(), conn.numpy(), bc.numpy(), P.Material(sigma_y=sigma_y, H=H), 0.5, None,
                     P.edge_loads(coords.numpy(), edges.numpy(), P.TRACTION))
    rng = np.random.default_rng(1)
    u = rng.normal(size=(prob.n, 2)) * 1e-6
    ep, al = rng.normal(size=(prob.mesh.ne, 3)) * 2e-6, np.abs(rng.normal(size=prob.mesh.ne)) * 5e-5
    return prob, u, ep, al


def test_assembled_gradient_and_tangent_by_differences_and_structure():
    prob, u, ep, al = small_problem()
    E, g, r = prob.energy(u, ep, al, 0.7)
    assert 0.1 <= r["plastic"].mean() <= 0.9
    K = prob.tangent(u, ep, al, 0.7)
    assert np.abs(K - K.T).max() <= 1e-12 * np.abs(K).max()
    assert np.linalg.eigvalsh(0.5 * (K + K.T))[0] > 0                     # H > 0: positive definite
    rng = np.random.default_rng(2)
    d = rng.normal(size=u.shape)
    h = 1e-11
    Ep, gp, _ = prob.energy(u + h * d, ep, al, 0.7)
    Em, gm, _ = prob.energy(u - h * d, ep, al, 0.7)
    Kd = (K @ d.reshape(-1)).reshape(-1, 2)
    e_K = np.abs((gp - gm) / (2 * h) - Kd).max() / np.abs(Kd).max()
    e_g = abs((Ep - Em) / (2 * h) - (g * d).sum()) / np.abs(g * d).sum()
    print("g", e_g, "K", e_K)
    assert e_K <= 1e-4 and e_g <= 1e-4


def test_a_yield_stress_out_of_reach_gives_the_plane_strain_elastic_operator():
    prob, u, ep, al = small_problem(sigma_y=1e30)
    mat = prob.mat
    K = prob.tangent(u, np.zeros_like(ep), np.zeros_like(al), 1.0)
    lam, mu = mat.lam, mat.mu
    C = np.array([[lam + 2 * mu, lam, 0], [lam, lam + 2 * mu, 0], [0, 0, 2 * mu]])         # tensor shear component
    Kel = prob.mesh.K(np.broadcast_to(C, (prob.mesh.ne, 3, 3)))[np.ix_(prob.fdof, prob.fdof)]
    assert np.abs(K - Kel).max() <= 1e-13 * np.abs(Kel).max()
    r = prob.point(u, np.zeros_like(ep), np.zeros_like(al), 1.0)
    assert not r["plastic"].any() and (r["theta"] == 1).all() and (r["theta_bar"] == 0).all()


def test_a_proportional_path_in_one_step_equals_ten_sub_steps():
    mat = P.Material(sigma_y=1e5, H=5e8)
    rng = np.random.default_rng(4)
    eps = rng.normal(size=(200, 3)) * 4e-5
    z3, z1 = np.zeros((200, 3)), np.zeros(200)
    one = P.return_map(eps, z3, z1, mat)
    assert 0.3 <= one["plastic"].mean() <= 1.0
    ep, al = z3, z1
    for k in range(1, 11):
        r = P.return_map(eps * (k / 10), ep, al, mat)
        ep, al = r["ep"], r["al"]
    scale = np.abs(one["ep"]).max()
    assert np.abs(ep - one["ep"]).max() <= 1e-12 * scale and np.abs(al - one["al"]).max() <= 1e-12 * np.abs(one["al"]).max()
    assert np.abs(r["sig"] - one["sig"]).max() <= 1e-12 * np.abs(one["sig"]).max()


@pytest.mark.parametrize("name", list(P.CANTILEVERS))
def test_cantilever_paths_load_unload_and_reverse(name):
    prob = P.cantilever(name)[1]
    res = P.cantilever_path(name)
    frac = [r.plastic.mean() for r in res]
    print(name, "plastic fraction per step", [f"{f:.3f}" for f in frac], "newton", [r.newton_iterations for r in res],
          "cg", [r.cg_iterations for r in res], "steps", [[h["step"] for h in r.history] for r in res])
    assert all(r.converged for r in res)
    assert 0.1 <= max(frac[:4]) <= 0.9                                    # peak
    assert frac[4] <= 0.01                                                # the first unloading step is elastic
    assert frac[7] >= 0.05                                                # reversed loading yields again
    # the truncated-PCG Newton and a direct-solve Newton end at the same equilibrium
    ex = P.path(prob, P.LOADS[:4], rtol=1e-10, exact=True)
    assert np.abs(ex[3].u - res[3].u).max() <= 1e-6 * np.abs(ex[3].u).max()
