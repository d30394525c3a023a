"""r-adaptive QUAD4 solve (hidenn_fem_amd/radapt.py Quad4RAdaptiveSolver, csrc/mesh_guard.hip): the element measure and the
step bound against the numpy closed forms of tests/test_radapt_quad4_host.py, the quality barrier against autograd of the same
formula, the reduced coordinate gradient against the dense QUAD4 oracle, the bilinear patch test, the alternating run's
contract (monotone objective, no inversion, untouched rows and .grad) and example 4's --quad path.  Tolerances are those of the
TRI3 twin (test_gpu_radapt.py)."""
import math
import re

import numpy as np
import pytest
import torch

from test_gpu_radapt import _caller_rows
from test_gpu_solve_quad4 import _dense_solve, _lf, _model, _oracle
from test_radapt_quad4_host import quad4_corners_np, quad4_measure_np, quad4_step_bound_np

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")


def _perturb(m, scale, seed):
    """Random interior move, uniform in +-scale h per coordinate with h = (smallest |c_k|) / (longest edge).  An edge vector
    then changes by at most 2 sqrt(2) scale h, and a corner cross product by less than (4 sqrt(2) scale + 8 scale^2) of the
    smallest one (0.65 of it at scale 0.1): every cell stays valid, by construction and not by luck."""
    g = torch.Generator().manual_seed(seed)
    c, S = quad4_corners_np(_caller_rows(m)[m.connectivity.cpu().numpy()])
    h = np.abs(c).min() / math.sqrt(S.max())
    with torch.no_grad():
        step = (2.0 * torch.rand(m.node_coords_free.shape, generator=g, dtype=F64) - 1.0) * (scale * h)
        m.node_coords_free.add_(step.to(DEV, m.node_coords_free.dtype))


def _check_measure(m, tol=1e-13):
    from hidenn_fem_amd.radapt import quad4_mesh_quality
    mq = quad4_mesh_quality(m)
    conn = m.connectivity.cpu().numpy()
    q, r, inv = quad4_measure_np(_caller_rows(m)[conn], m.initial_node_coords.double().cpu().numpy()[conn])
    gq, gr = mq.q.cpu().numpy(), mq.det_ratio.cpu().numpy()
    assert gq.shape == q.shape and gr.shape == r.shape
    assert np.abs(gq - q).max() <= tol * np.abs(q).max()
    assert np.abs(gr - r).max() <= tol * np.abs(r).max()
    assert abs(mq.min_q - q.min()) <= tol * abs(q.min()) and abs(mq.min_det_ratio - r.min()) <= tol * abs(r.min())
    assert mq.min_q == gq.min() and mq.min_det_ratio == gr.min()            # the device reduction is exact
    assert mq.n_inverted == int(inv.sum())
    return mq, q


def _clockwise(nx=23, ny=17, jitter=0.25, seed=4):
    """The base mesh with every cell numbered clockwise (local nodes 0, 3, 2, 1)."""
    from hidenn_fem_amd.mesh import structured_quad_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = structured_quad_mesh(nx, ny, jitter=jitter, seed=seed, dtype=F64)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nc, conn[:, [0, 3, 2, 1]].contiguous(), boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                    neumann_edges=edges).to(DEV)


MESHES = {"base": lambda: _model(), "tile": lambda: _model(nx=61, ny=41, reorder="tile"),
          "f32": lambda: _model(nx=61, ny=41, dtype=torch.float32)}


# ---------------------------------------------------------------- 1. measure
@pytest.mark.parametrize("which", ["base", "tile", "f32", "clockwise"])
def test_measure_matches_numpy(which):
    m = _clockwise() if which == "clockwise" else MESHES[which]()
    if which == "base":
        assert m.Nelems == 352                                # two workgroups, the second one partial
    if which == "tile":
        assert m.row_order == "tile"
    mq, q = _check_measure(m)
    assert mq.n_inverted == 0 and mq.min_q > 0.0 and mq.min_det_ratio == 1.0
    assert (q > 0).all()                                      # clockwise cells too: q carries the sign of the initial area
    _perturb(m, 0.1, seed=len(which))
    mq, _ = _check_measure(m)
    assert mq.n_inverted == 0
    # push one interior node out of its star: through an opposite edge
    X = _caller_rows(m)
    row = len(m._idx_free) // 2
    j = int(m._idx_free[row])
    conn = m.connectivity.cpu().numpy()
    star = np.unique(conn[(conn == j).any(axis=1)])
    far = X[j] + 3.0 * np.ptp(X[star], axis=0).max() * np.array([0.6, 0.8])
    with torch.no_grad():
        m.node_coords_free[row] = torch.tensor(far, dtype=m.node_coords_free.dtype, device=DEV)
    mq, _ = _check_measure(m)
    assert mq.n_inverted >= 1 and mq.min_q <= 0.0


# ---------------------------------------------------------------- 2. step bound
@pytest.mark.parametrize("which", ["base", "tile", "f32"])
def test_step_bound_matches_numpy_and_lands_on_eta(which):
    from hidenn_fem_amd.radapt import quad4_max_feasible_step
    m = MESHES[which]()
    conn = m.connectivity.cpu().numpy()
    g = torch.Generator().manual_seed(5)
    for eta in (0.25, 0.6):
        for k in range(3):
            d = torch.randn(m.node_coords_free.shape, generator=g, dtype=F64).to(DEV) * 10.0 ** (k - 1)
            got = quad4_max_feasible_step(m, d, eta=eta)
            X, D = _caller_rows(m), _caller_rows(m, d)
            want = quad4_step_bound_np(X[conn], D[conn], eta)[0].min()
            assert math.isfinite(got) and abs(got - want) <= 1e-12 * want, (eta, k, got, want)
            c0, _ = quad4_corners_np(X[conn])
            c1, _ = quad4_corners_np((X + got * D)[conn])
            assert abs((c1 / c0).min() - eta) <= 1e-10, (eta, (c1 / c0).min())
            t = quad4_max_feasible_step(m, d, eta=eta, as_tensor=True)
            assert t.is_cuda and t.dtype == F64 and t.item() == got       # deterministic
    assert quad4_max_feasible_step(m, torch.zeros_like(m.node_coords_free)) == math.inf


# ---------------------------------------------------------------- 3. barrier
def _barrier_torch(X, Xr, conn, idx_free, weight):
    """Q = (w / (4 Ne)) sum_e sum_k (1 / q_ek - 1) and dQ/d(rows idx_free of X) by autograd on the CPU; X, Xr [Nn, 2] fp64."""
    xf = X[idx_free].clone().requires_grad_(True)
    full = X.clone()
    full[idx_free] = xf
    P, R = full[conn], Xr[conn]
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]

    def corners(T):
        a, b = torch.roll(T, -1, dims=1) - T, torch.roll(T, 1, dims=1) - T
        return cross(a, b), (a ** 2).sum(dim=-1) + (b ** 2).sum(dim=-1)

    c, S = corners(P)
    cr, _ = corners(R)
    s = torch.sign(cr[:, 0] + cr[:, 2])[:, None]
    q = 2.0 * s * c / S
    Q = weight / (4.0 * conn.shape[0]) * (1.0 / q - 1.0).sum()
    (g,) = torch.autograd.grad(Q, xf)
    return Q.item(), g


@pytest.mark.parametrize("which", ["base", "tile", "clockwise"])
def test_barrier_value_and_gradient_match_autograd(which):
    from hidenn_fem_amd.radapt import quad4_quality_barrier
    m = _clockwise() if which == "clockwise" else MESHES[which]()
    _perturb(m, 0.05, seed=9)
    w = 0.7
    val, g = quad4_quality_barrier(m, w)
    want_v, want_g = _barrier_torch(m.coords.detach().double().cpu(), m.initial_node_coords.double().cpu(),
                                    m.connectivity.cpu(), m._idx_free.long().cpu(), w)
    assert want_v > 0.0
    assert abs(val.item() - want_v) <= 1e-11 * abs(want_v)
    assert (g.cpu() - want_g).abs().max().item() <= 1e-11 * want_g.abs().max().item()      # storage order, as idx_free


# ---------------------------------------------------------------- 4. reduced gradient
@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_reduced_gradient_matches_the_dense_oracle(conv):
    from oracle import quad4 as Q, ref_chain as R
    from test_gpu_solve_quad4 import BASE, _mesh
    from hidenn_fem_amd.radapt import Quad4RAdaptiveSolver
    H, f, shp = _oracle(conv)
    ustar = _dense_solve(conv, H, f).reshape(shp)
    nc, conn, geom, bc, mn, edges = _mesh(**BASE)
    n = nc.shape[0]
    xq = nc[~geom].clone().requires_grad_(True)
    X = R.assemble_coords(n, ~geom, xq, geom, nc[geom])
    U = R.assemble_u(n, ~bc, ustar, bc, torch.tensor(0.0, dtype=F64))
    e = Q.quad4_domain_energy(X, U, conn, R.plane_stress_C(), None, conv) - R.edge_energy(X, U, edges, *R.interval_gauss(2))
    (want,) = torch.autograd.grad(e, xq)
    m = _model(conv=conv)
    s = Quad4RAdaptiveSolver(m, _lf(), cg_rtol=1e-13)
    # at the solver's own u (CG to 1e-13), then at the dense u* itself
    assert s.solver.solve().converged
    for k in range(2):
        ev, _, got = s.objective_and_grad()
        got = m.to_caller_order(got.reshape(-1, 2), "x").cpu()
        err = (got - want).abs().max().item() / want.abs().max().item()
        print(f"reduced gradient ({conv}, {'CG u' if k == 0 else 'dense u*'}): max err / max|g| = {err:.3e}")
        assert err <= 1e-8
        assert abs(ev - e.item()) <= 1e-10 * abs(e.item())
        with torch.no_grad():
            m.u_free.copy_(m.from_caller_order(ustar.to(DEV), "u"))
    assert m.node_coords_free.grad is None and m.u_free.grad is None


def test_central_difference_of_the_reduced_energy_matches_g_dot_d():
    from hidenn_fem_amd.radapt import Quad4RAdaptiveSolver
    m = _model()
    s = Quad4RAdaptiveSolver(m, _lf(), cg_rtol=1e-13)
    s.solver.solve()
    _, _, g = s.objective_and_grad()
    x0 = m.node_coords_free.detach().clone()
    d = torch.randn(x0.shape, generator=torch.Generator().manual_seed(3), dtype=F64).to(DEV)
    h = 1e-3 * min(s.mesh.step_bound(d, 0.25).item(), 1.0)

    def pistar(a):
        with torch.no_grad():
            m.node_coords_free.copy_(x0 + a * d)
        assert s.solver.solve().converged
        return s.objective()

    fd = (pistar(h) - pistar(-h)) / (2.0 * h)
    gd = torch.dot(g, d.reshape(-1)).item()
    print(f"central difference {fd:.9e} vs g.d {gd:.9e}")
    assert abs(fd - gd) <= 1e-5 * abs(gd), (fd, gd)


# ---------------------------------------------------------------- 5. patch test
def test_patch_test_stops_at_iteration_zero_with_the_constant_strain_energy():
    from oracle import quad4 as Q, ref_chain as R
    from hidenn_fem_amd.mesh import structured_quad_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.radapt import Quad4RAdaptiveSolver
    nc, conn, geom, bc, mn, edges = structured_quad_mesh(25, 15, length=2.0, height=1.0, jitter=0.3, seed=4, dtype=F64)
    A = torch.tensor([[1.0e-4, 3.0e-5], [3.0e-5, -2.0e-5]], dtype=F64)          # constant symmetric strain
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=geom.clone(), u_fixed=0.0).to(DEV)
    m.grad_convention = "physical"
    m.u_fixed = (nc[geom] @ A.T).to(DEV)                                         # u = A x on every boundary node
    x0, xfix0 = m.node_coords_free.detach().clone(), m.node_coords_fixed.clone()
    info = Quad4RAdaptiveSolver(m, _lf(), cg_rtol=1e-13).run()
    assert info.reason == "gtol" and info.iterations == 0, info
    assert torch.equal(m.node_coords_free.detach(), x0) and torch.equal(m.node_coords_fixed, xfix0)
    want = Q.quad4_domain_energy(nc, nc @ A.T, conn, R.plane_stress_C(), None, "physical").item()   # the exact field
    print(f"patch test: energy {info.energy[0]:.15e} oracle {want:.15e} |g_x|inf {info.grad_inf[0]:.3e}")
    assert abs(info.energy[0] - want) <= 1e-10 * abs(want), (info.energy[0], want)


# ---------------------------------------------------------------- 6. r-adaptive run
def _plate(dtype=F64):
    """41 x 21 nodes, left edge clamped, the default traction on the right edge."""
    return _model(nx=41, ny=21, jitter=0.2, seed=1, dtype=dtype)


@pytest.mark.parametrize("quality_weight", [0.0, 0.05])
def test_r_adaptive_run_lowers_the_reduced_energy_without_inverting(quality_weight):
    from hidenn_fem_amd.radapt import Quad4RAdaptiveSolver, quad4_mesh_quality
    m = _plate()
    assert m.Nelems == 800 and m.N_edges == 20
    lf = _lf()
    xfix0, ufull_dir0 = m.node_coords_fixed.clone(), m.u_full.detach()[m.dirichlet_mask].clone()
    assert m.node_coords_free.grad is None and m.u_free.grad is None
    eta = 0.25
    s = Quad4RAdaptiveSolver(m, lf, eta=eta, quality_weight=quality_weight, cg_rtol=1e-10, max_outer=15)
    info = s.run()
    print(f"run (w = {quality_weight}): {info.iterations} outer iterations ({info.reason}), energy {info.energy[0]:.9e} -> "
          f"{info.energy[-1]:.9e}, min q {info.min_q[0]:.4f} -> {info.min_q[-1]:.4f}, CG {info.cg_iterations}, "
          f"step ratios {[round(r, 4) for r in info.step_ratio[1:]]}")
    assert info.iterations >= 3, info
    f = info.objective
    for a, b in zip(f, f[1:]):
        assert b <= a + 1e-12 * abs(a), f
    assert info.energy[-1] < info.energy[0], info.energy
    assert all(r >= eta * (1.0 - 1e-12) for r in info.step_ratio[1:]), info.step_ratio
    assert all(0.0 < a <= 0.9 * am for a, am in zip(info.alpha[1:], info.alpha_max[1:]))
    mq = quad4_mesh_quality(m)
    assert mq.n_inverted == 0 and mq.min_q > 0.0
    assert torch.equal(m.node_coords_fixed, xfix0) and torch.equal(m.u_full.detach()[m.dirichlet_mask], ufull_dir0)
    assert m.node_coords_free.grad is None and m.u_free.grad is None


def test_r_adaptive_run_on_an_fp32_model_keeps_every_element_valid():
    from hidenn_fem_amd.radapt import quad4_mesh_quality, r_adapt_
    m = _plate(dtype=torch.float32)
    info = r_adapt_(m, _lf(torch.float32), max_outer=15)
    print(f"fp32 run: {info.iterations} outer iterations ({info.reason}), step ratios {info.step_ratio[1:]}")
    assert info.iterations >= 1 and m.node_coords_free.dtype == torch.float32
    assert quad4_mesh_quality(m).n_inverted == 0
    assert all(r >= 0.25 * (1.0 - 1e-6) for r in info.step_ratio[1:]), info.step_ratio


# ---------------------------------------------------------------- 7. example
def test_example4_quad_r_adapt_ends_below_the_frozen_mesh_energy(capsys):
    import examples.example4 as e4
    m, final = e4.run(nx=40, ny=20, dtype=F64, quad=True, r_adapt=True, outer=5)
    out = capsys.readouterr().out
    assert m.nodes_per_element == 4
    frozen = float(re.search(r"frozen-mesh energy (\S+)", out).group(1))
    adapted = float(re.search(r"r-adapted energy (\S+)", out).group(1))
    assert re.search(r"inverted elements 0\b", out), out
    assert adapted < frozen and abs(adapted - final) <= 1e-9 * abs(final), out
