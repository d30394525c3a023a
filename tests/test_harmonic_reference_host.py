"""tests/harmonic_reference.py against numpy.linalg.solve on small random SPD pencils (no GPU): the numpy COCG with each kind of
preconditioner, its stopping and breakdown rules, and the modal sum for Rayleigh damping."""
import numpy as np
import pytest
import scipy.linalg

import harmonic_reference as HR


def _pencil(n, seed):
    """A random SPD pencil (K, M) of even order n with the spectrum of K / M spread over two decades."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    K = (Q * np.geomspace(1.0, 100.0, n)) @ Q.T
    B = rng.standard_normal((n, n))
    M = B @ B.T / n + 0.5 * np.eye(n)
    return 0.5 * (K + K.T), 0.5 * (M + M.T)


@pytest.mark.parametrize("precond", ["none", "block_jacobi", "exact_shift"])
@pytest.mark.parametrize("n,seed", [(2, 0), (10, 1), (40, 2)])
def test_numpy_cocg_agrees_with_the_dense_solve(n, seed, precond):
    K, M = _pencil(n, seed)
    lam = scipy.linalg.eigh(K, M, eigvals_only=True)
    rng = np.random.default_rng(10 + seed)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    w1 = np.sqrt(lam[0])
    ray = HR.rayleigh_for(0.02, w1, np.sqrt(lam[-1]))
    for omega, rayleigh in ((0.0, ray), (0.5 * w1, ray), (w1, ray), (np.sqrt(np.sqrt(lam[0] * lam[-1])), ray),
                            (np.sqrt(0.5 * (lam[0] + lam[1])) if n > 2 else 2.0 * w1, (0.0, 0.0))):
        A = HR.dense_operator(K, M, omega, rayleigh)
        assert np.abs(A - A.T).max() == 0.0                       # complex symmetric, not Hermitian
        S = K + omega * omega * M
        T = {"none": None, "block_jacobi": HR.block_jacobi(S), "exact_shift": lambda r, S=S: np.linalg.solve(S, r)}[precond]
        x, info = HR.cocg(A, b, T=T, rtol=1e-10, max_iter=20 * n)
        ref = np.linalg.solve(A, b)
        smin = np.linalg.svd(A, compute_uv=False)[-1]
        assert info["converged"] and info["reason"] == "rtol", (omega, info)
        assert info["residual"] <= 1e-10 * info["rhs_norm"]
        assert info["true_residual"] <= 2e-10 * info["rhs_norm"] + 1e-13 * np.linalg.norm(A, 2) * np.linalg.norm(x)
        assert np.linalg.norm(x - ref) <= 2.0 * (info["true_residual"] + np.linalg.norm(b - A @ ref)) / smin + 1e-15
        # a warm start at the solution stops without an iteration
        _, again = HR.cocg(A, b, T=T, x0=ref, rtol=1e-8, max_iter=20 * n)
        assert again["iterations"] == 0 and again["converged"]


def test_numpy_cocg_stopping_and_breakdown_rules():
    K, M = _pencil(10, 3)
    A = HR.dense_operator(K, M, 1.0, (0.1, 0.01))
    b = np.arange(1.0, 11.0).astype(complex)
    _, info = HR.cocg(A, b, rtol=1e-12, max_iter=3)
    assert info["reason"] == "max_iter" and info["iterations"] == 3 and not info["converged"]
    _, info = HR.cocg(A, b, rtol=0.0, atol=1e-6 * np.linalg.norm(b), max_iter=200)
    assert info["reason"] == "atol" and info["converged"]
    x, info = HR.cocg(A, np.zeros(10), rtol=1e-8)
    assert info["iterations"] == 0 and info["converged"] and not x.any()
    # mu = p^T A p = 0 on the first direction: A = [[1, 0], [0, -1]], b = (1, 1): breakdown before x moves
    x, info = HR.cocg(np.diag([1.0, -1.0]).astype(complex), np.ones(2), rtol=1e-8)
    assert info["reason"] == "breakdown" and info["iterations"] == 0 and not x.any()
    # rho = r^T r = 0 with r != 0: b = (1, i) is isotropic in the unconjugated form
    x, info = HR.cocg(np.eye(2, dtype=complex), np.array([1.0, 1.0j]), rtol=1e-8)
    assert info["reason"] == "breakdown" and info["iterations"] == 0 and not x.any()
    _, info = HR.cocg(np.full((2, 2), np.nan, dtype=complex), np.ones(2), rtol=1e-8)
    assert info["reason"] == "breakdown"


@pytest.mark.parametrize("n,seed", [(2, 4), (12, 5), (40, 6)])
def test_modal_sum_equals_the_dense_solve_for_rayleigh_damping(n, seed):
    K, M = _pencil(n, seed)
    lam, Phi = scipy.linalg.eigh(K, M)
    assert np.abs(Phi.T @ M @ Phi - np.eye(n)).max() <= 1e-12
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    w1 = np.sqrt(lam[0])
    ray = HR.rayleigh_for(0.02, w1, np.sqrt(lam[min(2, n - 1)]))
    alpha_r, beta_r = ray
    assert abs(alpha_r / (2 * w1) + beta_r * w1 / 2 - 0.02) <= 1e-15
    for omega in (0.0, 0.5 * w1, w1, np.sqrt(np.sqrt(lam[0] * lam[-1]))):
        A = HR.dense_operator(K, M, omega, ray)
        ref = np.linalg.solve(A, b)
        got = HR.modal_sum(lam, Phi, b, omega, ray)
        cond = np.linalg.cond(A) * np.linalg.cond(M)
        assert np.linalg.norm(got - ref) <= 1e-15 * cond * np.linalg.norm(ref) * 10, omega
    # the coefficients: z_M carries the density, the dense operator takes M with it
    zk, zm = HR.coefficients(3.0, rho=2.0, rayleigh=(0.5, 0.25), eta=0.125)
    assert zk == complex(1.0, 0.875) and zm == complex(-18.0, 3.0)
