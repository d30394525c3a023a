"""Linear buckling by block LOBPCG on the pencil (K_G, K) (hidenn_fem_amd/buckling.py, csrc/buckling.hip) against
``scipy.linalg.eigh(K_G, K)``.

K = ``assemble_stiffness(model, loss_fn).to_dense()`` (pinned against the oracle Hessian by the AMG tests), K_G from
tests/buckling_reference.py at the model's own ``u_full``; both over the free u rows in storage order.  All norms are recomputed
in numpy from the dense matrices, in the form of ``test_gpu_modal.check`` with K in the role of the mass:

(a) ``converged``;
(b) ||K_G x_j - theta_j K x_j||_2 <= 2 rtol |theta_j| ||K x_j||_2;
(c) |X^T K X - I| <= 1e-10;
(d) index-wise |theta_j - theta_j^ref| <= ||r_j||_{K^-1} / ||x_j||_K + 1e-12 |theta_j|.

Iteration caps are conditions: ``amg`` within the default ``max_iter = 200``, ``block_jacobi`` within 2000 (the dense emulation
of tests/test_buckling_host.py needs 25-47 with the exact K^-1 and 310-659 with block Jacobi on the same plates)."""
import numpy as np
import pytest
import scipy.linalg
import torch

import buckling_reference as BR
import cg_reference

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")
RTOL, N_MODES = 1e-8, 4
U_FIXED = [3e-6, -2e-6]
_cache = {}


def make_model(kind, nx=None, ny=None, dtype=F64, reorder="auto", jitter=0.25, u_fixed=0.0):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    quad = kind == "quad4"
    gen, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nx, ny = (nx or 23), (ny or (19 if quad else 17))
    nc, conn, geom, bc, mn, edges = gen(nx, ny, jitter=jitter, dtype=dtype)
    m = cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=u_fixed, neumann_edges=edges, reorder=reorder)
    return m.to(DEV)


def make_loss(conv, dtype=F64):
    from hidenn_fem_amd.loss import EnergyLoss2D
    return EnergyLoss2D(device=DEV, dtype=dtype, grad_convention=conv)


def load_(model, lf, sign=-1.0):
    """The static state under the default traction (sign = +1) or the same traction reversed into compression (-1)."""
    from hidenn_fem_amd.solve import solve_displacement_
    info = solve_displacement_(model, lf, t_force=(lambda x: sign * lf.uniform_edge_force(x)), rtol=1e-12)
    assert info.converged
    return model


def dense_kg(model, lf, conv, dtype=np.float64):
    """K_G over the free u rows in storage order at the model's current u_full (widened to fp64)."""
    G = BR.geometric_stiffness(model.coords.detach().double().cpu().numpy(), model.connectivity.cpu().numpy(),
                               model.u_full.detach().double().cpu().numpy(), lf._mat, lf._W, conv, dtype)
    return BR.free_scalar(G, model._idx_ufree.cpu().numpy())


def dense_pencil(model, lf, conv):
    from hidenn_fem_amd.solve import assemble_stiffness
    K = assemble_stiffness(model, lf).to_dense().cpu().numpy()
    KG = dense_kg(model, lf, conv)
    return 0.5 * (KG + KG.T), 0.5 * (K + K.T)


def reference(kind, conv, sign=-1.0):
    """The dense pencil of one loaded plate and its lowest pairs: computed once, shared, never modified."""
    key = (kind, conv, sign)
    if key not in _cache:
        lf = make_loss(conv)
        KG, K = dense_pencil(load_(make_model(kind), lf, sign), lf, conv)
        _cache[key] = (KG, K, scipy.linalg.eigh(KG, K, eigvals_only=True, subset_by_index=[0, N_MODES - 1]))
    return _cache[key]


def check(info, KG, K, w_ref, rtol=RTOL, what=""):
    th = info.theta.numpy()
    X = info.modes.detach().cpu().numpy().reshape(th.shape[0], -1).T
    assert info.modes.dtype == F64 and info.theta.dtype == F64 and info.load_factors.dtype == F64
    assert info.converged, f"{what}: not converged in {info.iterations} iterations"                       # (a)
    assert (np.diff(th) >= 0).all()
    R = KG @ X - (K @ X) * th[None, :]
    rn, kn = np.linalg.norm(R, axis=0), np.linalg.norm(K @ X, axis=0)
    orth = np.abs(X.T @ K @ X - np.eye(th.shape[0])).max()
    bound = np.sqrt(np.einsum("ij,ij->j", R, np.linalg.solve(K, R))) / np.sqrt(np.einsum("ij,ij->j", X, K @ X)) + 1e-12 * np.abs(th)
    err = np.abs(th - w_ref[:th.shape[0]])
    print(what, f"it {info.iterations} res/(|theta| |Kx|) {(rn / (np.abs(th) * kn)).max():.2e} orth {orth:.1e} "
                f"max |dtheta|/bound {(err / bound).max():.2e} |dtheta|/|theta| {(err / np.abs(th)).max():.1e} "
                f"load factors {info.load_factors.numpy()}")
    assert (rn <= 2 * rtol * np.abs(th) * kn).all()                                                         # (b)
    assert orth <= 1e-10                                                                                    # (c)
    assert (err <= bound).all(), (th, w_ref)                                                                # (d)
    rec = info.residual_norms.numpy()
    assert rec.shape == th.shape and np.isfinite(rec).all() and (rec <= 2 * rtol * np.abs(th) * kn).all()
    lf = info.load_factors.numpy()
    neg = th < 0
    assert np.array_equal(np.isinf(lf), ~neg) and (lf[~neg] > 0).all()
    assert np.array_equal(lf[neg], -1.0 / th[neg]) and info.n_buckling == int(neg.sum())


# ---------------------------------------------------------------- the operator
@pytest.mark.parametrize("reorder", ["off", "auto"])
@pytest.mark.parametrize("conv", ["reference", "physical"])
@pytest.mark.parametrize("kind,nx,ny", [("tri3", 7, 5), ("tri3", 23, 17), ("quad4", 7, 5), ("quad4", 23, 19)])
def test_geometric_stiffness_apply_against_the_longdouble_reference(kind, nx, ny, conv, reorder):
    """``max|got - want| <= 16 d_ref + 1e-13 max|want|``: ``want`` is the longdouble product of the dense reference, ``d_ref``
    what the same reference in float64 deviates from it (the conditioning of this u_0: sigma_0 is a difference of displacements
    divided by a cell size); 16 covers another summation order, FMA contraction and the reciprocal-plus-Newton division of
    hfem_device.h.  Widths: one column, a ragged tile, a full tile, a chunk boundary (8 + 1), the largest basis."""
    from hidenn_fem_amd.buckling import BucklingSolver
    cg_reference.assert_longdouble_is_wider()
    lf = make_loss(conv)
    model = load_(make_model(kind, nx, ny, reorder=reorder, u_fixed=U_FIXED), lf)
    assert float(model.u_full.detach()[model._idx_udir.long()].abs().min()) > 0
    s = BucklingSolver(model, lf, n_modes=2, precond="block_jacobi")
    ops = BR.both_precisions(model.coords.detach().cpu().numpy(), model.connectivity.cpu().numpy(),
                             model.u_full.detach().cpu().numpy(), lf._mat, lf._W, conv, model._idx_ufree.cpu().numpy())
    for m in (1, 3, 8, 9, 24):
        V = np.random.default_rng(m).standard_normal((m, s.n_u, 2))
        Vd = torch.from_numpy(V).to(DEV)
        want, d_ref = BR.apply_both(ops, V)
        got = s.geometric_stiffness_apply(Vd)
        err = np.abs(got.cpu().numpy() - want).max()
        print(kind, nx, ny, conv, reorder, f"m={m} d_ref {d_ref:.2e} err {err:.2e} max|want| {np.abs(want).max():.2e}")
        assert got.shape == Vd.shape and got.dtype == F64
        assert err <= 16 * d_ref + 1e-13 * np.abs(want).max()
        assert torch.equal(got, s.geometric_stiffness_apply(Vd))           # bit-identical
    with pytest.raises(ValueError, match="block"):
        s.geometric_stiffness_apply(Vd[:, :-1].contiguous())
    with pytest.raises(ValueError, match="block"):
        s.geometric_stiffness_apply(torch.zeros((25, s.n_u, 2), dtype=F64, device=DEV))
    # stiffness_apply keeps meaning K V
    from hidenn_fem_amd.solve import assemble_stiffness
    K = assemble_stiffness(model, lf).to_dense().cpu().numpy()
    V3 = Vd[:3].contiguous()
    wantK = (K @ V[:3].reshape(3, -1).T).T.reshape(3, s.n_u, 2)
    assert np.abs(s.stiffness_apply(V3).cpu().numpy() - wantK).max() <= 1e-11 * np.abs(wantK).max()


# ---------------------------------------------------------------- the solve
@pytest.mark.parametrize("kind,precond,conv", [("tri3", "amg", "physical"), ("tri3", "amg", "reference"),
                                               ("quad4", "amg", "physical"), ("quad4", "amg", "reference"),
                                               ("tri3", "block_jacobi", "physical"), ("quad4", "block_jacobi", "physical")])
def test_load_factors_against_dense_eigh(kind, precond, conv):
    from hidenn_fem_amd.buckling import BucklingSolver
    KG, K, w = reference(kind, conv)
    lf = make_loss(conv)
    kw = dict(max_iter=2000) if precond == "block_jacobi" else {}
    s = BucklingSolver(load_(make_model(kind), lf), lf, n_modes=N_MODES, precond=precond, rtol=RTOL, **kw)
    assert s.block == 6 and s.max_iter == (2000 if precond == "block_jacobi" else 200)
    info = s.solve()
    assert info.modes.shape == (N_MODES, s.n_u, 2) and info.theta.shape == (N_MODES,)
    check(info, KG, K, w, what=f"{kind} {precond} {conv}")
    assert info.n_buckling == 4 and (w < 0).all()


@pytest.mark.parametrize("kind,conv,max_iter", [("tri3", "physical", 1000), ("tri3", "reference", 200), ("quad4", "physical", 1000)])
def test_tension_gives_the_signs_of_the_dense_pencil(kind, conv, max_iter):
    """The unreversed default traction: the lowest theta are those of the dense pencil, sign included, and ``load_factors`` is
    ``inf`` exactly where theta >= 0 (``check``).  In the physical convention a plate in tension keeps only a handful of negative
    theta (6 of 748 on the TRI3 plate: the lateral contraction is restrained at the clamped edge) at the thin end of a spectrum
    that is positive almost everywhere, so the iteration is slow whatever the preconditioner: the dense emulation with the exact
    K^-1 needs 658 (TRI3) and 291 (QUAD4) iterations (tests/test_buckling_host.py), hence the cap of 1000 there."""
    from hidenn_fem_amd.buckling import linear_buckling
    KG, K, w = reference(kind, conv, sign=1.0)
    lf = make_loss(conv)
    info = linear_buckling(load_(make_model(kind), lf, sign=1.0), lf, n_modes=N_MODES, rtol=RTOL, max_iter=max_iter)
    check(info, KG, K, w, what=f"{kind} {conv} tension")
    assert np.array_equal(np.sign(info.theta.numpy()), np.sign(w))


def test_pure_tension_has_no_buckling_factor():
    """u_0 = alpha (x, 0) in the physical convention: sigma_xx, sigma_yy > 0 and sigma_xy = 0 in every element, so K_G is
    positive definite and EVERY Ritz value is positive, converged or not: no buckling mode, all factors inf, no error."""
    from hidenn_fem_amd.buckling import BucklingSolver
    model, lf = make_model("tri3"), make_loss("physical")
    with torch.no_grad():
        x = model.coords.detach()[model._idx_ufree.long()]
        model.u_free.copy_(torch.stack([1e-5 * x[:, 0], torch.zeros_like(x[:, 0])], dim=1))
    info = BucklingSolver(model, lf, n_modes=N_MODES, max_iter=3).solve()
    assert (info.theta.numpy() > 0).all() and info.n_buckling == 0
    assert np.isinf(info.load_factors.numpy()).all() and info.iterations <= 3


def test_doubling_the_prestress_halves_the_load_factors_and_the_model_is_untouched():
    from hidenn_fem_amd.buckling import BucklingSolver
    lf = make_loss("physical")
    m = load_(make_model("quad4"), lf)
    s = BucklingSolver(m, lf, n_modes=N_MODES, rtol=RTOL)
    before = {k: v.clone() for k, v in list(m.named_parameters()) + list(m.named_buffers())}
    state = {k: v.clone() for k, v in m.state_dict().items()}
    one = s.solve()
    KG, K, w = reference("quad4", "physical")
    check(one, KG, K, w, what="first solve")
    after = dict(list(m.named_parameters()) + list(m.named_buffers()))
    assert set(before) == set(after)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert m.u_free.grad is None and m.node_coords_free.grad is None
    # u_free changes in place: the next solve() notices by itself and rebuilds the prestress
    with torch.no_grad():
        m.u_free.mul_(2.0)
    two = s.solve()
    assert two.converged and two.n_buckling == 4
    l1, l2 = one.load_factors.numpy(), two.load_factors.numpy()
    print("load factors", l1, l2, f"max |2 l2 - l1| / l1 {(np.abs(2 * l2 - l1) / l1).max():.2e}")
    assert (np.abs(2.0 * l2 - l1) <= 1e-9 * l1).all()
    KG2, _ = dense_pencil(m, lf, "physical")
    check(two, KG2, K, 2.0 * w, what="doubled prestress")


def test_row_order_does_not_change_the_load_factors():
    """80 x 60 nodes: ``reorder="auto"`` stores the rows tile-major; the initial block is drawn in the caller's order."""
    from hidenn_fem_amd.buckling import BucklingSolver
    lf = make_loss("physical")
    out = {}
    for reorder in ("off", "auto"):
        m = load_(make_model("tri3", 80, 60, reorder=reorder), lf)
        s = BucklingSolver(m, lf, n_modes=N_MODES, rtol=RTOL, seed=7)
        info = s.solve()
        assert info.converged and info.n_buckling == 4
        out[reorder] = (m, s, info)
    assert out["auto"][0].row_order == "tile" and out["off"][0].row_order == "as given"
    to, ta = out["off"][2].theta.numpy(), out["auto"][2].theta.numpy()
    print(f"max |dtheta|/|theta| {(np.abs(to - ta) / np.abs(to)).max():.2e}; iterations {out['off'][2].iterations} / "
          f"{out['auto'][2].iterations}; load factors {out['off'][2].load_factors.numpy()}")
    assert (np.abs(to - ta) <= 1e-9 * np.abs(to)).all()
    xo, xa = (out[k][1].modes_in_caller_order().cpu().numpy().reshape(N_MODES, -1) for k in ("off", "auto"))
    cos = np.abs(np.einsum("ij,ij->i", xo, xa)) / (np.linalg.norm(xo, axis=1) * np.linalg.norm(xa, axis=1))
    assert (cos >= 1.0 - 1e-6).all(), cos


def test_fp32_model_gives_the_fp64_factors_of_its_widened_rows():
    from hidenn_fem_amd.buckling import linear_buckling
    lf = make_loss("physical", torch.float32)                 # ONE loss for both: an fp32 loss holds fp32-rounded material constants
    m32 = load_(make_model("tri3", dtype=torch.float32), lf)
    m64 = make_model("tri3", dtype=torch.float32).double()
    with torch.no_grad():
        m64.u_free.copy_(m32.u_free.detach().double())
    KG, K = dense_pencil(m64, lf, "physical")
    w = scipy.linalg.eigh(KG, K, eigvals_only=True, subset_by_index=[0, N_MODES - 1])
    info = linear_buckling(m32, lf, n_modes=N_MODES, rtol=RTOL)
    assert m32.u_free.dtype == torch.float32 and m32.node_coords_free.dtype == torch.float32
    check(info, KG, K, w, what="fp32 model")


def test_linear_buckling_with_its_own_static_solve():
    """``solve=True`` runs the static solve first (it writes ``u_free``); the traction of that solve is passed through."""
    from hidenn_fem_amd.buckling import linear_buckling
    lf = make_loss("physical")
    m = make_model("quad4")
    with torch.no_grad():
        m.u_free.zero_()
    info = linear_buckling(m, lf, solve=True, t_force=lambda x: -lf.uniform_edge_force(x), n_modes=N_MODES, rtol=RTOL)
    assert float(m.u_free.detach().abs().max()) > 0
    KG, K = dense_pencil(m, lf, "physical")                                # at the u_free that solve left behind
    check(info, KG, K, scipy.linalg.eigh(KG, K, eigvals_only=True, subset_by_index=[0, N_MODES - 1]), what="solve=True")
    assert info.n_buckling == 4
