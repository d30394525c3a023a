"""r-adaptive TRI3 solve (hidenn_fem_amd/radapt.py, csrc/mesh_guard.hip): the element measure and the step bound against numpy
closed forms, the quality barrier against autograd of the same formula, the reduced coordinate gradient against the dense
oracle, the P1 patch test, the alternating run's contract (monotone energy, no inversion, untouched rows and .grad), and the
example's --r-adapt path."""
import math
import re

import numpy as np
import pytest
import torch

from conftest import tri_mesh_dict
from test_radapt_host import _measure_np, step_bound_np

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")


def _caller_rows(m, d=None):
    """[Nn, 2] fp64 rows by node id: the model's current coordinates (d None) or a storage-order direction d (fixed rows 0)."""
    if d is None:
        with torch.no_grad():
            return m.coords.detach().double().cpu().numpy()
    out = np.zeros((m.Nnodes, 2))
    out[m._idx_free.cpu().numpy()] = d.detach().double().cpu().numpy()
    return out


def _perturb(m, scale, seed):
    """Random interior move of relative size `scale` of the local element size (keeps the mesh valid for small scale)."""
    g = torch.Generator().manual_seed(seed)
    X = _caller_rows(m)
    P = X[m.connectivity.cpu().numpy()]
    h = math.sqrt(np.abs((P[:, 0, 0] - P[:, 2, 0]) * (P[:, 1, 1] - P[:, 2, 1])
                         - (P[:, 1, 0] - P[:, 2, 0]) * (P[:, 0, 1] - P[:, 2, 1])).min())
    with torch.no_grad():
        step = torch.randn(m.node_coords_free.shape, generator=g, dtype=F64) * (scale * h)
        m.node_coords_free.add_(step.to(DEV, m.node_coords_free.dtype))


def _check_measure(m, tol=1e-13):
    from hidenn_fem_amd.radapt import mesh_quality
    mq = mesh_quality(m)
    conn = m.connectivity.cpu().numpy()
    q, r = _measure_np(_caller_rows(m), m.initial_node_coords.double().cpu().numpy(), conn)
    gq, gr = mq.q.cpu().numpy(), mq.det_ratio.cpu().numpy()
    assert np.abs(gq - q).max() <= tol * np.abs(q).max()
    assert np.abs(gr - r).max() <= tol * np.abs(r).max()
    assert abs(mq.min_q - q.min()) <= tol * abs(q.min()) and abs(mq.min_det_ratio - r.min()) <= tol * abs(r.min())
    assert mq.n_inverted == int((r <= 0).sum())
    return mq, q


# ---------------------------------------------------------------- 1. measure
def test_measure_matches_numpy_on_every_golden_case(g_tri):
    from test_gpu_parity import tri_model_from_golden
    for case in g_tri.cases():
        m = tri_model_from_golden(g_tri, case, DEV)
        mq, q = _check_measure(m)
        assert mq.n_inverted == 0 and mq.min_q > 0.0 and mq.min_det_ratio == 1.0, case
        if case == "flipped":
            assert (q > 0).all()                         # clockwise elements are valid: q uses the sign of the initial detJ
        _perturb(m, 0.1, seed=len(case))
        _check_measure(m)
    for case in ("permuted_random_diag", "order4"):     # push one interior node through its opposite edge: inverted elements
        m = tri_model_from_golden(g_tri, case, DEV)
        X = _caller_rows(m)
        row = len(m._idx_free) // 2
        j = int(m._idx_free[row])
        conn = m.connectivity.cpu().numpy()
        star = np.unique(conn[(conn == j).any(axis=1)])
        far = X[j] + 3.0 * np.ptp(X[star], axis=0).max() * np.array([0.6, 0.8])   # out of its star: through an opposite edge
        with torch.no_grad():
            m.node_coords_free[row] = torch.tensor(far, dtype=F64, device=DEV)
        mq, _ = _check_measure(m)
        assert mq.n_inverted >= 1 and mq.min_q <= 0.0, case


def _structured(reorder="auto", dtype=F64, nx=61, ny=41, jitter=0.25, seed=3, **kw):
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(nx, ny, jitter=jitter, seed=seed, dtype=F64, **kw)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nc.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                    neumann_edges=edges, reorder=reorder).to(DEV)


def test_measure_on_tile_major_rows_and_fp32_rows():
    m = _structured("tile")
    assert m.row_order == "tile"
    _perturb(m, 0.1, seed=1)
    _check_measure(m)
    m32 = _structured("auto", dtype=torch.float32)
    _perturb(m32, 0.1, seed=2)
    mq, _ = _check_measure(m32)
    assert mq.n_inverted == 0


# ---------------------------------------------------------------- 2. step bound
def _unstructured(dtype=F64, n=6000):
    from hidenn_fem_amd.mesh import unstructured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = unstructured_tri_mesh(n, dtype=F64)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nc.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                    neumann_edges=edges).to(DEV)


def _bound_np(m, d, eta):
    conn = m.connectivity.cpu().numpy()
    X, D = _caller_rows(m), _caller_rows(m, d)
    a, *_ = step_bound_np(X[conn], D[conn], eta)
    return a.min(), X, D, conn


@pytest.mark.parametrize("which", ["structured", "structured_tile", "unstructured", "structured_f32"])
def test_step_bound_matches_numpy_and_lands_on_eta(which):
    from hidenn_fem_amd.radapt import max_feasible_step
    m = {"structured": lambda: _structured("off"), "structured_tile": lambda: _structured("tile", nx=81, ny=61),
         "unstructured": _unstructured, "structured_f32": lambda: _structured("auto", dtype=torch.float32)}[which]()
    g = torch.Generator().manual_seed(5)
    for eta in (0.25, 0.6):
        for k in range(3):
            d = torch.randn(m.node_coords_free.shape, generator=g, dtype=F64).to(DEV) * 10.0 ** (k - 1)
            got = max_feasible_step(m, d, eta=eta)
            want, X, D, conn = _bound_np(m, d, eta)
            assert math.isfinite(got) and abs(got - want) <= 1e-12 * want, (eta, k, got, want)
            _, r = _measure_np(X + got * D, X, conn)
            assert abs(r.min() - eta) <= 1e-10, (eta, r.min())
            t = max_feasible_step(m, d, eta=eta, as_tensor=True)
            assert t.is_cuda and t.dtype == F64 and t.item() == got       # deterministic
    assert max_feasible_step(m, torch.zeros_like(m.node_coords_free)) == math.inf


def test_step_bound_of_a_single_node_pushed_toward_its_opposite_edge():
    from hidenn_fem_amd.radapt import max_feasible_step
    m = _structured("off", jitter=0.0)
    X = _caller_rows(m)
    conn = m.connectivity.cpu().numpy()
    row = len(m._idx_free) // 2
    j = int(m._idx_free[row])
    # the elements around j; the node moves straight at the opposite edge of the first one, at unit speed
    es = np.nonzero((conn == j).any(axis=1))[0]
    e = conn[es[0]]
    a, b = [X[n] for n in e if n != j]
    t = (b - a) / np.linalg.norm(b - a)
    foot = a + np.dot(X[j] - a, t) * t
    hgt = np.linalg.norm(X[j] - foot)
    dirn = (foot - X[j]) / hgt
    d = torch.zeros(m.node_coords_free.shape, dtype=F64)
    d[row] = torch.tensor(dirn)
    eta = 0.25
    got = max_feasible_step(m, d.to(DEV), eta=eta)
    # every element around j: detJ is linear in alpha (one corner moves); the first to reach eta of its area sets the bound
    want = math.inf
    for ee in es:
        P = X[conn[ee]]
        k = list(conn[ee]).index(j)
        o = [P[i] for i in range(3) if i != k]
        ed = o[1] - o[0]
        nrm = np.array([-ed[1], ed[0]]) / np.linalg.norm(ed)
        h0 = np.dot(P[k] - o[0], nrm)                    # signed height of j over the edge
        rate = np.dot(dirn, nrm)
        if rate * h0 < 0:
            want = min(want, (1.0 - eta) * abs(h0) / abs(rate))
    assert want <= (1.0 - eta) * hgt * (1.0 + 1e-12)              # the element straight ahead crosses there, others maybe sooner
    assert abs(got - want) <= 1e-12 * want, (got, want)


# ---------------------------------------------------------------- 3. barrier
def _barrier_torch(m, weight):
    X = m.coords.detach().double().cpu()
    Xr = m.initial_node_coords.double().cpu()
    conn = m.connectivity.cpu()
    idx_free = m._idx_free.long().cpu()
    xf = X[idx_free].clone().requires_grad_(True)
    full = X.clone()
    full[idx_free] = xf
    P, R = full[conn], Xr[conn]
    det = lambda T: (T[:, 0, 0] - T[:, 2, 0]) * (T[:, 1, 1] - T[:, 2, 1]) - (T[:, 1, 0] - T[:, 2, 0]) * (T[:, 0, 1] - T[:, 2, 1])
    S = sum(((P[:, (i + 1) % 3] - P[:, i]) ** 2).sum(dim=1) for i in range(3))
    q = 2.0 * math.sqrt(3.0) * torch.sign(det(R)) * det(P) / S
    Q = weight / conn.shape[0] * (1.0 / q - 1.0).sum()
    (g,) = torch.autograd.grad(Q, xf)
    return Q.item(), g


@pytest.mark.parametrize("which", ["flipped", "structured_tile", "unstructured"])
def test_barrier_value_and_gradient_match_autograd(g_tri, which):
    from hidenn_fem_amd.radapt import quality_barrier
    from test_gpu_parity import tri_model_from_golden
    m = {"flipped": lambda: tri_model_from_golden(g_tri, "flipped", DEV), "structured_tile": lambda: _structured("tile"),
         "unstructured": _unstructured}[which]()
    _perturb(m, 0.05, seed=9)
    w = 0.7
    val, g = quality_barrier(m, w)
    want_v, want_g = _barrier_torch(m, w)
    got_g = g.cpu()                                                  # storage order, as xf in _barrier_torch
    assert abs(val.item() - want_v) <= 1e-11 * abs(want_v)
    assert (got_g - want_g).abs().max().item() <= 1e-11 * want_g.abs().max().item()


# ---------------------------------------------------------------- 4. reduced gradient
def test_reduced_gradient_matches_the_dense_oracle(g_tri):
    from oracle.ref_chain import total_energy
    from test_gpu_solve import _dev_forces, _golden_model, _loss, _oracle, _solve_cases
    from hidenn_fem_amd.radapt import RAdaptiveSolver
    for case in _solve_cases(g_tri):
        H, f, shp = _oracle(g_tri, case, "reference")
        ustar = torch.linalg.solve(H, f).reshape(shp)
        mesh, xf, _ = tri_mesh_dict(g_tri, case)
        go, go1 = (int(v) for v in g_tri[case + "/gauss_order"])
        b, t, bd, td = _dev_forces(case)
        xq = xf.clone().requires_grad_(True)
        e = total_energy(xq, ustar, mesh, gauss_order=go, gauss_order_1d=go1, b_force=b, t_force=t)
        (want,) = torch.autograd.grad(e, xq)
        lf, _, _ = _loss(g_tri, case)
        m = _golden_model(g_tri, case)
        s = RAdaptiveSolver(m, lf, b_force=bd, t_force=td, cg_rtol=1e-13)
        assert s.solver.solve().converged
        _, _, got = s.objective_and_grad()
        got = m.to_caller_order(got.reshape(-1, 2), "x").cpu()
        assert (got - want).abs().max().item() <= 1e-8 * want.abs().max().item(), case


def test_central_difference_of_the_reduced_energy_matches_g_dot_d(g_tri):
    from test_gpu_solve import _golden_model, _loss
    from hidenn_fem_amd.radapt import RAdaptiveSolver
    case = "order4"
    lf, _, _ = _loss(g_tri, case)
    m = _golden_model(g_tri, case)
    s = RAdaptiveSolver(m, lf, cg_rtol=1e-13)
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
    assert abs(fd - gd) <= 1e-5 * abs(gd), (fd, gd)


# ---------------------------------------------------------------- 5. patch test
def test_patch_test_stops_at_iteration_zero_with_the_constant_strain_energy():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.radapt import RAdaptiveSolver
    L, Hh = 2.0, 1.0
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(25, 15, length=L, height=Hh, jitter=0.3, seed=4, diagonal="random",
                                                        dtype=F64)
    A = np.array([[1.0e-4, 3.0e-5], [3.0e-5, -2.0e-5]])              # constant symmetric strain
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=geom.clone(), u_fixed=0.0).to(DEV)
    m.grad_convention = "physical"
    bnd = np.nonzero(geom.numpy())[0]
    m.u_fixed = torch.tensor(nc.numpy()[bnd] @ A.T, dtype=F64, device=DEV)            # u = A x on every boundary node
    lf = EnergyLoss2D(device=DEV, dtype=F64)
    x0, xfix0 = m.node_coords_free.detach().clone(), m.node_coords_fixed.clone()
    info = RAdaptiveSolver(m, lf, cg_rtol=1e-13).run()
    assert info.reason == "gtol" and info.iterations == 0, info
    assert torch.equal(m.node_coords_free.detach(), x0) and torch.equal(m.node_coords_fixed, xfix0)
    c11, c12, c22, c33 = lf._mat
    eps = np.array([A[0, 0], A[1, 1], 2.0 * A[0, 1]])
    psi = 0.5 * (c11 * eps[0] ** 2 + 2.0 * c12 * eps[0] * eps[1] + c22 * eps[1] ** 2 + c33 * eps[2] ** 2)
    want = 2.0 * lf._W * (L * Hh) * psi                                 # sum |detJ| W psi, sum |detJ| = 2 x the area
    assert abs(info.energy[0] - want) <= 1e-10 * abs(want), (info.energy[0], want)


# ---------------------------------------------------------------- 6. r-adaptive run
def _plate(nx=60, ny=30, dtype=F64):
    from hidenn_fem_amd.mesh import generate_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nodes, conn, geom, bc, mn, edges = generate_mesh(2.0, 1.0, [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)],
                                                     {"up": 0, "down": 0, "right": 2, "left": 1}, nx, ny)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nodes.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                    neumann_edges=edges).to(DEV)


@pytest.mark.parametrize("quality_weight", [0.0, 0.05])
def test_r_adaptive_run_lowers_the_reduced_energy_without_inverting(quality_weight):
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.radapt import RAdaptiveSolver, mesh_quality
    m = _plate()
    assert 2000 <= m.Nelems <= 8000
    lf = EnergyLoss2D(device=DEV, dtype=F64)
    xfix0, ufull_dir0 = m.node_coords_fixed.clone(), m.u_full.detach()[m.dirichlet_mask].clone()
    assert m.node_coords_free.grad is None and m.u_free.grad is None
    eta, rtol = 0.25, 1e-10
    s = RAdaptiveSolver(m, lf, eta=eta, quality_weight=quality_weight, cg_rtol=rtol, max_outer=20)
    info = s.run()
    assert info.iterations >= 5, info
    f = info.objective
    for a, b in zip(f, f[1:]):
        assert b <= a + 1e-12 * abs(a), f
    assert info.energy[-1] < info.energy[0], info.energy
    assert all(r >= eta * (1.0 - 1e-12) for r in info.step_ratio[1:]), info.step_ratio
    assert all(0.0 < a <= 0.9 * am for a, am in zip(info.alpha[1:], info.alpha_max[1:]))
    mq = mesh_quality(m)
    assert mq.n_inverted == 0 and mq.min_q > 0.0
    assert torch.equal(m.node_coords_fixed, xfix0) and torch.equal(m.u_full.detach()[m.dirichlet_mask], ufull_dir0)
    assert m.node_coords_free.grad is None and m.u_free.grad is None
    with torch.enable_grad():
        (gu,) = torch.autograd.grad(lf(m), m.u_free)
    assert s.last_solve.converged, s.last_solve
    # the true residual at the end.  With the barrier the mesh stays shaped and CG reaches its tolerance.  Without it the energy
    # thins elements toward q -> 0: cond(K) grows with it and the fp64 gradient itself carries a rounding
    # floor (2e-6 to 4e-6 of ||f|| on this plate after 20 steps) that no CG restart gets under
    bound = 10.0 * rtol if quality_weight > 0.0 else 1e-4
    assert gu.norm().item() <= bound * s.last_solve.rhs_norm, (gu.norm().item(), s.last_solve, info.min_q)
    assert m.node_coords_free.grad is None and m.u_free.grad is None


def test_r_adaptive_run_on_an_fp32_model_keeps_every_element_valid():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.radapt import RAdaptiveSolver, mesh_quality
    m = _plate(dtype=torch.float32)
    info = RAdaptiveSolver(m, EnergyLoss2D(device=DEV, dtype=torch.float32), max_outer=20).run()
    assert info.iterations >= 1 and m.node_coords_free.dtype == torch.float32
    assert mesh_quality(m).n_inverted == 0
    assert all(r >= 0.25 * (1.0 - 1e-6) for r in info.step_ratio[1:]), info.step_ratio
    assert info.energy[-1] < info.energy[0]


# ---------------------------------------------------------------- 7. example
def test_example4_r_adapt_ends_below_the_frozen_mesh_energy(capsys):
    import examples.example4 as e4
    m, final = e4.run(nx=40, ny=20, dtype=F64, r_adapt=True, outer=5)
    out = capsys.readouterr().out
    frozen = float(re.search(r"frozen-mesh energy (\S+)", out).group(1))
    adapted = float(re.search(r"r-adapted energy (\S+)", out).group(1))
    assert re.search(r"inverted elements 0\b", out), out
    assert adapted < frozen and abs(adapted - final) <= 1e-9 * abs(final), out
