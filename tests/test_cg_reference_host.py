"""The references of tests/cg_reference.py against closed forms, without a GPU: they are what the GPU tests hold the PCG
driver and the V-cycle to, so they must not be wrong in the way a kernel could be.  The block-sparse products against dense
products, ``vcycle`` against the dense error-propagation form of a smoothed-aggregation cycle built from the Chebyshev
polynomial itself (not from the c1 / c2 recurrence), ``pcg_steps`` against ``torch.linalg.solve``, and the scalar coefficient
formulas against T_2 scaled to 1 at 0."""
import numpy as np
import pytest
import torch

import cg_reference as R

LD = np.longdouble
DTYPES = [np.float64, np.longdouble]


def test_longdouble_is_wider_than_double():
    R.assert_longdouble_is_wider()


# ---------------------------------------------------------------- block-sparse products
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rb,cb", [(1, 1), (2, 2), (3, 3), (2, 3)])
def test_block_products_equal_dense_products_with_empty_rows_and_rectangular_blocks(dtype, rb, cb):
    rng = np.random.default_rng(rb * 10 + cb)
    nb, nc = 17, 11
    keep = rng.random((nb, nc)) < 0.3
    keep[3] = False                                                  # empty rows, the last one too
    keep[nb - 1] = False
    dense = (rng.standard_normal((nb, rb, nc, cb)) * keep[:, None, :, None]).reshape(nb * rb, nc * cb).astype(dtype)
    A = R.Bsr.from_dense(dense, rb, cb)
    assert A.shape == dense.shape and A.vals.dtype == dtype and len(A.col) == keep.sum()
    x = rng.standard_normal(nc * cb).astype(dtype)
    y = rng.standard_normal(nb * rb).astype(dtype)
    tol = 8 * nc * cb * float(np.finfo(dtype).eps)                   # a row sums at most nc * cb products
    got = A.matvec(x)
    assert got.dtype == dtype and np.abs(got - dense @ x).max() <= tol * np.abs(dense).max() * np.abs(x).max()
    gt = A.transpose().matvec(y)
    assert gt.dtype == dtype and np.abs(gt - dense.T @ y).max() <= tol * nb / nc * np.abs(dense).max() * np.abs(y).max()
    assert np.array_equal(A.to_dense(), dense) and np.array_equal(A.transpose().to_dense(), dense.T)
    assert A.matvec(x.astype(np.float64)).dtype == dtype             # the wider of the two types
    if rb == cb:
        D = A.diagonal_blocks()
        for i in range(min(nb, nc)):
            assert np.array_equal(D[i], dense[i * rb:(i + 1) * rb, i * cb:(i + 1) * cb])
        want = np.concatenate([D[i] @ x[i * cb:(i + 1) * cb] for i in range(nc)])
        assert np.abs(R.block_diag_matvec(D[:nc], x) - want).max() <= tol * np.abs(dense).max() * np.abs(x).max()
    if rb == cb == 1:
        assert np.array_equal(R.csr_matvec(A.ptr, A.col, A.vals.reshape(-1), x), got)


# ---------------------------------------------------------------- the V-cycle against its dense closed form
def _hierarchy(nb=60):
    """A small SPD block problem and a smoothed-aggregation hierarchy on it, dense, in float64: a chain of ``nb`` nodes with 2x2
    blocks, aggregated by threes twice (60 -> 20 -> 7 block rows: three levels, 3x3 blocks below the fine one)."""
    rng = np.random.default_rng(7)
    lap = 2.0 * np.eye(nb) - np.eye(nb, k=1) - np.eye(nb, k=-1)
    A = np.kron(lap, np.array([[2.0, 0.5], [0.5, 1.0]]))
    for i in range(nb):                                              # diagonal blocks that differ from row to row
        g = rng.standard_normal((2, 2))
        A[2 * i:2 * i + 2, 2 * i:2 * i + 2] += 0.05 * (g @ g.T)
    xy = np.stack([np.linspace(0.0, 1.0, nb), 0.3 * np.sin(np.arange(nb))], axis=1)
    ns = np.zeros((nb, 2, 3))
    ns[:, 0, 0] = ns[:, 1, 1] = 1.0
    ns[:, 0, 2], ns[:, 1, 2] = -xy[:, 1], xy[:, 0]
    dense = []
    bs = 2
    while True:
        n = A.shape[0] // bs
        Dinv = np.stack([np.linalg.inv(A[i * bs:(i + 1) * bs, i * bs:(i + 1) * bs]) for i in range(n)])
        Dinv = 0.5 * (Dinv + Dinv.transpose(0, 2, 1))
        Dfull = np.zeros_like(A)
        for i in range(n):
            Dfull[i * bs:(i + 1) * bs, i * bs:(i + 1) * bs] = Dinv[i]
        if len(dense) == 2:
            return dense, A
        lam_true = np.linalg.eigvals(Dfull @ A).real.max()
        coef = R.cheb_coefficients(1.1 * lam_true)
        nagg = (n + 2) // 3
        T = np.zeros((n * bs, nagg * 3))
        ns_next = np.zeros((nagg, 3, 3))
        for J in range(nagg):
            rows = slice(3 * J * bs, min(3 * J + 3, n) * bs)
            Q, Rj = np.linalg.qr(ns.reshape(n * bs, 3)[rows])
            T[rows, 3 * J:3 * J + 3] = Q
            ns_next[J] = Rj
        P = T - coef["omega"] * (Dfull @ (A @ T))
        rec = np.zeros(8)
        rec[[R.K_LAM, R.K_INV_THETA, R.K_C1, R.K_C2, R.K_OMEGA]] = [1.1 * lam_true, coef["inv_theta"], coef["c1"], coef["c2"],
                                                                   coef["omega"]]
        dense.append(dict(A=A, Dinv=Dinv, Dfull=Dfull, P=P, coef=rec, bs=bs, theta=coef["theta"], delta=coef["delta"]))
        A = P.T @ A @ P
        A = 0.5 * (A + A.T)
        ns, bs = ns_next, 3


def _dense_cycle(dense, coarse_inv, level=0):
    """M_l = (I - E_l) A_l^-1 with E_l = S_l (I - P_l M_{l+1} P_l^T A_l) S_l and S = T_2((theta - G) / delta) / T_2(theta / delta),
    G = D^-1 A: the error propagation of two-step Chebyshev smoothing around a coarse correction, nested."""
    if level == len(dense):
        return coarse_inv
    L = dense[level]
    A, n = L["A"], L["A"].shape[0]
    I = np.eye(n)
    G = L["Dfull"] @ A
    Y = (L["theta"] * I - G) / L["delta"]
    sigma = L["theta"] / L["delta"]
    S = (2.0 * Y @ Y - I) / (2.0 * sigma * sigma - 1.0)
    Mc = _dense_cycle(dense, coarse_inv, level + 1)
    E = S @ (I - L["P"] @ Mc @ L["P"].T @ A) @ S
    return (I - E) @ np.linalg.inv(A)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nlev", [2, 3])
def test_vcycle_equals_the_dense_error_propagation_form_and_is_symmetric(dtype, nlev):
    dense, Ac = _hierarchy()
    assert [L["A"].shape[0] for L in dense] + [Ac.shape[0]] == [120, 60, 21] and [L["bs"] for L in dense] == [2, 3]
    if nlev == 2:                                                    # two levels: the 60-dof operator is the coarsest
        dense, Ac = dense[:1], dense[1]["A"]
    coarse_inv = np.linalg.inv(Ac)
    coarse_inv = 0.5 * (coarse_inv + coarse_inv.T)
    M = _dense_cycle(dense, coarse_inv)
    levels = R.cast_levels([dict(A=R.Bsr.from_dense(L["A"], L["bs"], L["bs"]), Dinv=L["Dinv"], coef=L["coef"],
                                 P=R.Bsr.from_dense(L["P"], L["bs"], 3)) for L in dense], dtype)
    n = dense[0]["A"].shape[0]
    got = np.stack([R.vcycle(levels, coarse_inv, e, dtype) for e in np.eye(n)], axis=1)
    assert got.dtype == dtype
    # the dense form inverts A in float64: its relative error is at most n eps cond(A) (the bound for an explicit inverse)
    cond = np.linalg.cond(dense[0]["A"])
    tol = n * R.EPS64 * cond
    err = R.rel(got, M)
    print(f"vcycle vs dense form ({nlev} levels, {np.dtype(dtype).name}): {err:.3e} (bound {tol:.3e}, cond {cond:.3e})")
    assert tol < 1e-9 and err <= tol
    assert R.rel(got.T, got) <= tol and R.rel(M.T, M) <= tol
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0
    if dtype == LD:                                                  # the float64 run is the longdouble run up to rounding
        lo = R.cast_levels(levels, np.float64)
        b = np.random.default_rng(1).standard_normal(n)
        dev = R.rel(R.vcycle(lo, coarse_inv, b, np.float64), R.vcycle(levels, coarse_inv, b, LD))
        assert 0.0 < dev <= 1e3 * R.EPS64 * cond


# ---------------------------------------------------------------- pcg_steps against torch.linalg.solve
def _spd(n=40, seed=3):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, 50.0, n)) @ Q.T
    return 0.5 * (A + A.T), rng.standard_normal(n), rng.standard_normal(n)


def test_pcg_steps_without_a_preconditioner_converges_to_the_dense_solution():
    A, f, u0 = _spd()
    n, ns = len(f), 100                                             # cond 50: 0.75 per step at worst
    want = torch.linalg.solve(torch.from_numpy(A), torch.from_numpy(f)).numpy()
    g0 = A @ u0 - f                                                  # dE/du at u0 for E = 1/2 u^T A u - f^T u; at 0 it is -f
    steps = R.pcg_steps(A, None, g0, -f, ns, LD, u0=u0)
    assert len(steps) == ns + 1 and [s["iter"] for s in steps] == list(range(ns + 1))
    assert steps[0]["beta"] == 0 and np.array_equal(steps[0]["u"], u0.astype(LD))
    assert abs(steps[0]["fnorm"] - np.linalg.norm(f)) <= 4 * R.EPS64 * np.linalg.norm(f)
    tol = n * R.EPS64 * np.linalg.cond(A)                            # the accuracy of the fp64 LU solve it is compared with
    assert R.rel(steps[-1]["u"], want) <= tol
    rn = [float(s["rnorm"]) for s in steps]
    assert rn[-1] <= 1e-12 * rn[0]
    for s in steps[1:]:                                              # the recursion's |r| is the true residual in longdouble
        true = np.linalg.norm((f.astype(LD) - A.astype(LD) @ s["u"]).astype(np.float64))
        assert abs(true - float(s["rnorm"])) <= 1e-12 * rn[0]
        assert abs(s["alpha"] * s["pq"] - steps[s["iter"] - 1]["rho"]) <= 4 * R.EPS64 * abs(steps[s["iter"] - 1]["rho"])
        assert abs(s["beta"] * steps[s["iter"] - 1]["rho"] - s["rho"]) <= 4 * R.EPS64 * abs(s["rho"])
    lo = R.pcg_steps(A, None, g0, -f, 6, np.float64, u0=u0)
    dev = R.pcg_deviation(lo, steps[:7])
    assert all(0.0 < dev[-1][q] < 1e-10 for q in R.SCALARS + ("u",)) and dev[0]["alpha"] == 0.0
    assert all(dev[k][q] <= dev[k + 1][q] for k in range(6) for q in dev[0])


def test_pcg_steps_with_the_exact_inverse_as_preconditioner_is_done_after_one_step():
    A, f, u0 = _spd()
    n = len(f)
    want = torch.linalg.solve(torch.from_numpy(A), torch.from_numpy(f)).numpy()
    Ainv = np.linalg.inv(A)
    tol = n * R.EPS64 * np.linalg.cond(A)
    for M in (Ainv, lambda r: Ainv.astype(r.dtype) @ r):             # a dense array and a callable
        steps = R.pcg_steps(A, M, A @ u0 - f, -f, 2, LD, u0=u0)
        assert R.rel(steps[1]["u"], want) <= tol
        assert abs(steps[1]["alpha"] - 1.0) <= tol and steps[1]["rnorm"] <= tol * steps[0]["rnorm"]


def test_block_jacobi_restatement_inverts_the_blocks_and_falls_back_to_the_identity():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((6, 2, 2))
    B = g @ g.transpose(0, 2, 1) + 0.1 * np.eye(2)
    diag = np.stack([B[:, 0, 0], B[:, 0, 1], B[:, 1, 1]], axis=1)
    diag[4] = [1.0, 2.0, 1.0]                                        # not positive definite: identity
    r = rng.standard_normal(12)
    for dtype in DTYPES:
        z = R.block_jacobi(diag, dtype)(r.astype(dtype)).reshape(6, 2)
        assert z.dtype == dtype
        for i in range(6):
            want = r[2 * i:2 * i + 2] if i == 4 else np.linalg.solve(B[i], r[2 * i:2 * i + 2])
            assert np.abs(z[i] - want).max() <= 64 * R.EPS64 * np.linalg.cond(B[i]) * np.abs(want).max()
        assert np.array_equal(R.block_jacobi(diag, dtype, identity=True)(r.astype(dtype)), r.astype(dtype))


# ---------------------------------------------------------------- scalar coefficients
@pytest.mark.parametrize("lam", [0.37, 1.0, 1.9, 2.6])
def test_coefficients_reproduce_the_degree_two_chebyshev_residual_polynomial(lam):
    """T_2 mapped to [lam / 30, lam] and scaled to 1 at 0: p(t) = T_2((theta - t) / delta) / T_2(theta / delta)."""
    c = R.cheb_coefficients(lam, LD)
    lo, hi = LD(lam) / 30, LD(lam)
    assert c["lo"] == lo and abs(c["theta"] - (hi + lo) / 2) <= 2e-19 * hi and abs(c["delta"] - (hi - lo) / 2) <= 2e-19 * hi
    assert abs(c["omega"] - LD(4) / (3 * hi)) <= 2e-19 * c["omega"]
    assert abs(c["c1"] - c["rho1"] * c["rho0"]) == 0 and abs(c["c2"] - 2 * c["rho1"] / c["delta"]) == 0
    t2 = lambda x: 2 * x * x - 1
    sigma = c["theta"] / c["delta"]
    top = 1 / t2(sigma)
    pts = [LD(0), lo, c["theta"], hi, 0.1 * hi, 0.5 * hi, 0.77 * hi, 1.05 * hi]
    for t in pts:
        want = t2((c["theta"] - t) / c["delta"]) / t2(sigma)
        assert abs(R.cheb_residual_polynomial(c, t) - want) <= 64 * float(np.finfo(LD).eps), (lam, t)
    p = lambda t: R.cheb_residual_polynomial(c, t)
    assert p(LD(0)) == 1
    assert abs(p(lo) - top) <= 1e-17 and abs(p(hi) - top) <= 1e-17 and abs(p(c["theta"]) + top) <= 1e-17   # equioscillation
    assert all(abs(p(lo + (hi - lo) * s)) <= top * (1 + 1e-15) for s in np.linspace(0.0, 1.0, 41).astype(LD))
    c64 = R.cheb_coefficients(lam, np.float64)                       # the float64 record is the longdouble one rounded
    for k in c:
        assert isinstance(c64[k], np.float64) and abs(LD(c64[k]) - c[k]) <= 8 * R.EPS64 * abs(c[k]), k


def test_allowed_is_thirty_two_deviations_plus_sixty_four_eps():
    assert R.allowed(0.0) == 64 * R.EPS64 and R.allowed(1e-12) == 32e-12 + 64 * R.EPS64
