"""The smoothed-aggregation V-cycle of the frozen-mesh solve (csrc/tri3_amg.hip) and its ingredients, level by level, on a
TRI3 and a QUAD4 mesh with three levels each: D^-1 against the adjugate inverse in longdouble, the coefficient record against
the formulas of amg_power_finish_kernel, lambda_hat against the true lambda_max(D^-1 A), the coarsest inverse, the QUAD4 twin
of the numpy restatement of P / near-null space / A_c (the first check of the npe = 4 path below the fine level), the cycle
itself against ``cg_reference.vcycle`` on the arrays read back from the device, and the single-level hierarchy, whose cycle
is the dense solve."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import cg_reference as R
from cg_reference import _bsr, _mgs, _power
from test_gpu_solve import _golden_model, _loss, _oracle, _structured
from test_gpu_solve_quad4 import BASE, _lf, _model as _quad_model, _oracle as _quad_oracle

pytestmark = pytest.mark.gpu
F64 = torch.float64
LD = np.longdouble
DEV = torch.device("cuda:0")
CONVS = ["reference", "physical"]
# the smallest mesh of the family nx x (nx + 1) / 2 (the base mesh's jitter and seed) whose host hierarchy has three levels,
# found on the CPU with amg_host: 93 x 47 stops at two (4324 -> 473 block rows), 97 x 49 gives 4704 -> 541 -> 53
QUAD3 = dict(nx=97, ny=49, jitter=0.25, seed=4)
TRI_SINGLE = "permuted_random_diag"


def _solver(kind, conv):
    """An AMG solver after its refresh on the three-level mesh of ``kind``."""
    from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver
    if kind == "tri3":
        m = _structured("auto", nx=121, ny=61)
        m.grad_convention = conv
        s = FrozenMeshSolver(m, _lf(), precond="amg")
    else:
        m = _quad_model(conv=conv, **QUAD3)
        s = Quad4FrozenMeshSolver(m, _lf(), precond="amg")
    s.refresh()
    assert len(s._amg.host.levels) >= 3, s.amg
    if kind == "quad4":
        assert s.amg["block_rows"] == [4704, 541, 53], s.amg
    return s


def device_levels(s):
    """The hierarchy as ``cg_reference.vcycle`` takes it, from the arrays read back from the device (float64), and the
    coarsest inverse."""
    a, host = s._amg, s._amg.host
    out = []
    for lvl in range(len(host.levels) - 1):
        n, bs = host.levels[lvl][:2]
        nagg = host.levels[lvl][3]
        out.append(dict(A=R.Bsr(a.values(lvl, 0).cpu().numpy(), host.array(lvl, 0), host.array(lvl, 1), bs, bs, n),
                        Dinv=a.values(lvl, 1).cpu().numpy().reshape(n, bs, bs), coef=a.values(lvl, 2).cpu().numpy(),
                        P=R.Bsr(a.values(lvl, 5).cpu().numpy(), host.array(lvl, 4), host.array(lvl, 5), bs, 3, nagg)))
    return out, a.coarse_inv.cpu().numpy()


def _level_matrix(s, lvl):
    a, host = s._amg, s._amg.host
    n, bs = host.levels[lvl][:2]
    return R.Bsr(a.values(lvl, 0).cpu().numpy(), host.array(lvl, 0), host.array(lvl, 1), bs, bs, n)


# ---------------------------------------------------------------- D^-1
def _adjugate_inverse(B):
    """Closed-form inverse of [n, bs, bs] blocks (bs 2 or 3) in their own type; det <= 0 or non-finite gives the identity."""
    n, bs, _ = B.shape
    if bs == 2:
        adj = np.empty_like(B)
        adj[:, 0, 0], adj[:, 1, 1] = B[:, 1, 1], B[:, 0, 0]
        adj[:, 0, 1], adj[:, 1, 0] = -B[:, 0, 1], -B[:, 1, 0]
        det = B[:, 0, 0] * B[:, 1, 1] - B[:, 0, 1] * B[:, 1, 0]
    else:
        adj = np.empty_like(B)
        for r in range(3):
            for c in range(3):                                       # adj[r][c] = cofactor of entry (c, r)
                r1, r2 = (c + 1) % 3, (c + 2) % 3
                c1, c2 = (r + 1) % 3, (r + 2) % 3
                adj[:, r, c] = B[:, r1, c1] * B[:, r2, c2] - B[:, r1, c2] * B[:, r2, c1]
        det = B[:, 0, 0] * adj[:, 0, 0] + B[:, 0, 1] * adj[:, 1, 0] + B[:, 0, 2] * adj[:, 2, 0]
    ok = (det > 0) & np.isfinite(det)
    inv = adj / np.where(ok, det, 1)[:, None, None]
    inv[~ok] = np.eye(bs, dtype=B.dtype)
    return inv, ok


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_dinv_is_the_inverse_of_the_symmetrised_diagonal_block_on_every_level(kind, conv):
    """values(level, 1) against the adjugate inverse in longdouble of 1/2 (B + B^T) with a zero diagonal entry replaced by 1
    (amg_dinv_kernel), both block sizes.  Bound per block: 16 bs eps cond_2(B) max|B^-1|.  An explicit inverse from a
    forward-stable method satisfies |X - B^-1| <= c bs eps |B^-1| |B| |B^-1| (Higham, Accuracy and Stability, ch. 14), normwise
    c bs eps cond(B) |B^-1|; c counts the roundings on the longest path to an entry -- for bs = 3 a cofactor (3), the
    determinant on top of it (5), the reciprocal, the product and the symmetrising average (2): 12, taken as 16."""
    R.assert_longdouble_is_wider()
    s = _solver(kind, conv)
    host = s._amg.host
    sizes = set()
    for lvl in range(len(host.levels)):
        n, bs = host.levels[lvl][:2]
        sizes.add(bs)
        B = _level_matrix(s, lvl).diagonal_blocks()
        B = 0.5 * (B + B.transpose(0, 2, 1))
        idx = np.arange(bs)
        zero = B[:, idx, idx] == 0.0
        B[:, idx, idx] = np.where(zero, 1.0, B[:, idx, idx])
        want, ok = _adjugate_inverse(B.astype(LD))
        got = s._amg.values(lvl, 1).cpu().numpy().reshape(n, bs, bs)
        cond = np.linalg.cond(B)
        err = np.abs(got.astype(LD) - want).max(axis=(1, 2)).astype(np.float64)
        bound = 16 * bs * R.EPS64 * cond * np.abs(want).max(axis=(1, 2)).astype(np.float64)
        worst = int(np.argmax(err / bound))
        print(f"dinv ({kind}, {conv}) level {lvl} bs {bs}: {n} blocks, {int(zero.sum())} zero diagonal entries replaced, "
              f"{int((~ok).sum())} identity fallbacks, max cond {cond.max():.3e}, max err / bound {err[worst] / bound[worst]:.3e}")
        assert np.all(err <= bound), (lvl, worst, err[worst], bound[worst])
        assert np.array_equal(got, got.transpose(0, 2, 1)), lvl       # stored symmetrised
    assert sizes == {2, 3}


# ---------------------------------------------------------------- the coefficient record
# relative error of each scalar in unit roundoffs u = eps / 2, every operation correctly rounded (first order):
#   lo = lam / 30: 1; theta = 0.5 (lam + lo): the sum's rounding + lo's share (1 / 31) < 2; delta: < 2 likewise;
#   1 / theta: 3; sigma = theta / delta: 5; rho0 = 1 / sigma: 6; 2 sigma - rho0 with sigma = 31 / 29, rho0 = 29 / 31 (the
#   difference is 1.20): (2 * 1.069 * 5 + 0.935 * 6) / 1.20 + 1 < 15; rho1: 16; c1 = rho1 rho0: 16 + 6 + 1 = 23;
#   c2 = 2 rho1 / delta: 16 + 2 + 1 = 19; omega = 4 / (3 lam): 2
COEF_ROUNDOFFS = {"inv_theta": 3, "c1": 23, "c2": 19, "omega": 2}


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_coefficient_record_follows_the_formulas_and_the_interval_covers_the_spectrum(kind, conv):
    """kInvTheta, kC1, kC2, kOmega recomputed from coef[kLam] (exactly, in longdouble) within the roundoff count of
    COEF_ROUNDOFFS; coef[kLam] == 1.1 coef[kNorm]; and coef[kLam] >= lambda_max(D^-1 A), the largest eigenvalue of
    D^-1/2 A D^-1/2 (dense below 2000 dofs, else Lanczos): the Chebyshev interval must cover the spectrum."""
    R.assert_longdouble_is_wider()
    s = _solver(kind, conv)
    host = s._amg.host
    u = 0.5 * R.EPS64
    for lvl in range(len(host.levels) - 1):
        n, bs = host.levels[lvl][:2]
        coef = s._amg.values(lvl, 2).cpu().numpy()
        lam = coef[R.K_LAM]
        assert lam > 0.0 and lam == 1.1 * coef[R.K_NORM], (lvl, coef)
        exact, same = R.cheb_coefficients(lam, LD), R.cheb_coefficients(lam, np.float64)
        for name, slot in (("inv_theta", R.K_INV_THETA), ("c1", R.K_C1), ("c2", R.K_C2), ("omega", R.K_OMEGA)):
            err = float(abs(LD(coef[slot]) - exact[name]) / abs(exact[name]))
            print(f"coef ({kind}, {conv}) level {lvl} {name}: {coef[slot]!r}, error {err / u:.2f} u (allowed "
                  f"{COEF_ROUNDOFFS[name]} u), equal to the float64 restatement: {coef[slot] == same[name]}")
            assert err <= COEF_ROUNDOFFS[name] * u, (lvl, name, coef[slot], exact[name])
        A = _bsr(s._amg.values(lvl, 0).cpu().numpy(), host.array(lvl, 0), host.array(lvl, 1), bs, bs, n)
        Dinv = s._amg.values(lvl, 1).cpu().numpy().reshape(n, bs, bs)
        w, V = np.linalg.eigh(Dinv)
        assert w.min() > 0.0, lvl
        half = sp.block_diag(list((V * np.sqrt(w)[:, None, :]) @ V.transpose(0, 2, 1))).tocsr()
        S = (half @ A @ half).tocsr()
        S = 0.5 * (S + S.T)
        if n * bs <= 2000:
            lam_max = np.linalg.eigvalsh(S.toarray())[-1]
        else:
            lam_max = spla.eigsh(S, k=1, which="LA", tol=1e-10, ncv=40)[0][0]
        print(f"lambda ({kind}, {conv}) level {lvl}: lambda_hat {lam:.6f}, lambda_max(D^-1 A) {lam_max:.6f}, "
              f"ratio {lam / lam_max:.4f}, power estimate / lambda_max {coef[R.K_NORM] / lam_max:.4f}")
        assert lam >= lam_max, (lvl, lam, lam_max)


# ---------------------------------------------------------------- the coarsest inverse
@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_coarse_inverse_is_exactly_symmetric_and_inverts_the_coarsest_operator(kind, conv):
    """``A_c`` from values(last, 0) scattered to dense (an all-zero row gets a 1 on its diagonal, as the scatter kernel does).
    max|A_c X - I| <= N eps cond_2(A_c): the residual bound of an inverse computed by LU, |A X - I| <= c N u |L| |U| |X|
    (Higham, ch. 14), with |L| |U| |X| bounded by cond(A_c); symmetrising averages the left and the right residual."""
    s = _solver(kind, conv)
    X = s._amg.coarse_inv
    assert torch.equal(X, X.T)
    last = len(s._amg.host.levels) - 1
    Ac = _level_matrix(s, last).to_dense()
    N = Ac.shape[0]
    assert X.shape == (N, N) and N <= 1500
    zero = ~np.any(Ac != 0.0, axis=1)
    Ac[zero, zero] = 1.0
    assert np.array_equal(Ac, s._amg.coarse.cpu().numpy())
    cond = np.linalg.cond(Ac)
    res = np.abs(Ac.astype(LD) @ X.cpu().numpy().astype(LD) - np.eye(N, dtype=LD)).max()
    print(f"coarse inverse ({kind}, {conv}): N {N}, {int(zero.sum())} zero rows, cond {cond:.3e}, max|A X - I| {float(res):.3e}, "
          f"bound {N * R.EPS64 * cond:.3e}")
    assert res <= N * R.EPS64 * cond


# ---------------------------------------------------------------- QUAD4 twin of the level restatement
@pytest.mark.parametrize("conv", CONVS)
def test_every_quad4_level_matches_a_numpy_restatement_and_coarse_operators_are_symmetric(conv):
    """test_gpu_amg.py's restatement of the numeric setup on a QUAD4 hierarchy (9-point fan, npe = 4), with its bounds."""
    s = _solver("quad4", conv)
    a, host = s._amg, s._amg.host
    nlev = len(host.levels)
    assert nlev >= 3
    for lvl in range(nlev - 1):
        n, bs = host.levels[lvl][:2]
        nagg = host.levels[lvl][3]
        A = _bsr(a.values(lvl, 0).cpu().numpy(), host.array(lvl, 0), host.array(lvl, 1), bs, bs, n)
        blocks = [A[i * bs:(i + 1) * bs, i * bs:(i + 1) * bs].toarray() for i in range(n)]
        inv = []
        for Bk in blocks:
            Bk = 0.5 * (Bk + Bk.T)
            Bk[np.diag(Bk) == 0.0, np.diag(Bk) == 0.0] = 1.0
            inv.append(np.linalg.inv(Bk))
        Dinv = sp.block_diag(inv).tocsr()
        lam = _power(A, Dinv, n * bs)
        coef = a.values(lvl, 2).cpu().numpy()
        assert abs(coef[0] - lam) <= 1e-8 * lam, (lvl, coef[0], lam)
        omega = coef[4]
        ns = a.values(lvl, 3).cpu().numpy().reshape(n, bs, 3)
        agg = host.array(lvl, 3)
        T = np.zeros((n, bs, 3))
        Rn = np.zeros((nagg, 3, 3))
        for J in range(nagg):
            mem = np.nonzero(agg == J)[0]
            Q, Rj = _mgs(ns[mem].reshape(-1, 3))
            T[mem] = Q.reshape(len(mem), bs, 3)
            Rn[J] = Rj
        Tm = _bsr(T.reshape(-1), np.arange(n + 1), agg, bs, 3, nagg)
        P = (Tm - omega * (Dinv @ (A @ Tm))).tocsr()
        Pd = _bsr(a.values(lvl, 5).cpu().numpy(), host.array(lvl, 4), host.array(lvl, 5), bs, 3, nagg)
        scale = abs(P).max()
        assert abs(Pd - P).max() <= 1e-12 * scale, lvl
        ns_next = a.values(lvl + 1, 3).cpu().numpy().reshape(nagg, 3, 3)
        assert np.abs(ns_next - Rn).max() <= 1e-12 * np.abs(Rn).max(), lvl
        Ac = (P.T @ A @ P).tocsr()
        Acd = _bsr(a.values(lvl + 1, 0).cpu().numpy(), host.array(lvl + 1, 0), host.array(lvl + 1, 1), 3, 3, nagg)
        assert abs(Acd - Ac).max() <= 1e-12 * abs(Ac).max(), lvl
        assert abs(Acd - Acd.T).max() <= 1e-12 * abs(Acd).max(), lvl
    rep = s.amg
    assert rep["levels"] == nlev and rep["operator_complexity"] > 1.0 and rep["host_setup_seconds"] > 0.0


# ---------------------------------------------------------------- the cycle
def _spike_rows(m):
    """Storage rows of a free node that shares an element with a Dirichlet node, and of the free node nearest the centre."""
    conn = m.connectivity.detach().cpu().numpy()
    dmask = m.dirichlet_mask.detach().cpu().numpy().astype(bool)
    xy = m.initial_node_coords.detach().cpu().numpy()
    u_src = np.asarray(m._u_src)
    touching = conn[dmask[conn].any(axis=1)].reshape(-1)
    near = int(touching[~dmask[touching]][0])
    far_from = np.where(dmask, np.inf, np.linalg.norm(xy - 0.5 * (xy.min(axis=0) + xy.max(axis=0)), axis=1))
    centre = int(np.argmin(far_from))
    assert u_src[near] >= 0 and u_src[centre] >= 0 and not dmask[conn[(conn == centre).any(axis=1)]].any()
    return int(u_src[near]), int(u_src[centre])


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_vcycle_equals_the_reference_cycle_on_the_device_arrays(kind, conv):
    """``precondition(r)`` against ``cg_reference.vcycle`` in longdouble on A, D^-1, coef, P and coarse_inv as read back from
    the device, for a random r, a spike beside a Dirichlet row, a spike in the interior, and r = 0 (z exactly 0).  The kernel
    may deviate ``allowed`` x what the float64 run of the same reference deviates from the longdouble run, relative to
    max|z|.  The arrays themselves are held to references by the tests above and the level restatements."""
    R.assert_longdouble_is_wider()
    s = _solver(kind, conv)
    m = s.model
    levels, coarse_inv = device_levels(s)
    hi, lo = R.cast_levels(levels, LD), R.cast_levels(levels, np.float64)
    n = m.u_free.shape[0]
    near, centre = _spike_rows(m)
    torch.manual_seed(11)
    rs = {"random": torch.randn((n, 2), dtype=F64, device=DEV), "zero": torch.zeros((n, 2), dtype=F64, device=DEV)}
    for name, row in (("spike_dirichlet", near), ("spike_interior", centre)):
        rs[name] = torch.zeros((n, 2), dtype=F64, device=DEV)
        rs[name][row] = torch.tensor([1.0, -0.5], dtype=F64, device=DEV)
    for name, r in rs.items():
        z = s.precondition(r).cpu().numpy().reshape(-1)
        if name == "zero":
            assert np.all(z == 0.0)
            continue
        b = r.cpu().numpy().reshape(-1)
        want = R.vcycle(hi, coarse_inv, b, LD)
        dev = R.rel(R.vcycle(lo, coarse_inv, b, np.float64), want)
        got = R.rel(z, want)
        print(f"vcycle ({kind}, {conv}, {name}): reference float64 vs longdouble {dev:.3e}, kernel vs longdouble {got:.3e}, "
              f"allowed {R.allowed(dev):.3e}")
        assert np.abs(want).max() > 0 and got <= R.allowed(dev), (name, got, dev)


# ---------------------------------------------------------------- a single level: the cycle is the dense solve
def _storage_order(m, H):
    """The caller-order dense Hessian over the rows of ``u_free`` as stored."""
    n = m.u_free.shape[0]
    perm = m.to_caller_order(torch.arange(n, device=m.u_free.device), "u").cpu()      # caller row k <- storage row perm[k]
    inv = torch.argsort(perm)                                                       # storage row s -> caller row inv[s]
    return H.reshape(n, 2, n, 2)[inv][:, :, inv].reshape(2 * n, 2 * n)


def _checked_solve(H, r):
    """``H^-1 r`` by LU with the accuracy check of test_gpu_solve_quad4._dense_solve (normwise backward error <= 3e-15), and
    cond_2(H): the relative error of the result is at most cond(H) x that."""
    u = torch.linalg.solve(H, r)
    eta = (H @ u - r).norm().item() / (torch.linalg.matrix_norm(H, 2).item() * u.norm().item())
    assert eta <= 3e-15, eta
    return u, torch.linalg.cond(H).item()


def _single(kind, conv, g_tri):
    from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver
    if kind == "tri3":
        H, f, shp = _oracle(g_tri, TRI_SINGLE, conv)
        m = _golden_model(g_tri, TRI_SINGLE, conv=conv)
        lf, _, _ = _loss(g_tri, TRI_SINGLE)
        from test_gpu_solve import _dev_forces
        _, _, bd, td = _dev_forces(TRI_SINGLE)
        mk = lambda **kw: FrozenMeshSolver(m, lf, b_force=bd, t_force=td, precond="amg", **kw)
    else:
        H, f, shp = _quad_oracle(conv)
        m = _quad_model(conv=conv, **BASE)
        mk = lambda **kw: Quad4FrozenMeshSolver(m, _lf(), precond="amg", **kw)
    return m, _storage_order(m, H), m.from_caller_order(f.reshape(shp), "u").reshape(-1), mk


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_single_level_cycle_is_the_dense_oracle_solve_and_pcg_needs_two_iterations_at_most(g_tri, kind, conv):
    m, H, f, mk = _single(kind, conv, g_tri)
    s = mk(rtol=1e-10)
    assert s.amg["levels"] == 1, s.amg
    torch.manual_seed(2)
    for name, r in (("f", f), ("random", torch.randn(f.shape, dtype=F64))):
        want, cond = _checked_solve(H, r)
        z = s.precondition(r.reshape(-1, 2).to(DEV)).cpu().reshape(-1)
        err = (z - want).norm().item() / want.norm().item()
        print(f"single level ({kind}, {conv}, {name}): |M r - H^-1 r| / |H^-1 r| = {err:.3e}, bound cond(H) 3e-15 = {cond * 3e-15:.3e}")
        assert err <= cond * 3e-15, (name, err, cond)
    info = s.solve()
    print(f"single level ({kind}, {conv}): {info}")
    assert info.converged and info.reason == "rtol" and info.iterations <= 2, info
