"""Element-scaled solves and the SIMP design loop (hidenn_fem_amd/topopt.py) on the plates of
tests/test_gpu_modal.py (23 x 17 TRI3, 23 x 19 QUAD4) against tests/topopt_reference.py.

Scaled solve: ``|u_dev - u_ref| <= 2 (|r_dev| + |r_ref|) / lambda_min(K(w))`` against a sparse direct solve, residuals
recomputed in numpy from the reference K(w) -- the bound the project uses for its other solves.  Compliance and sensitivity:
1e-10 relative to the reference formulas evaluated at the device's own u.  Loop: 25 ``step()``s under the conditions of
tests/test_topopt_reference_host.py::reference_loop; volume, bounds and flag at every step, the compliance decreasing at every
step and ``c_25 <= 0.5 c_1``.  The two loops make the same decisions only up to rounding, so the distance of their final
compliances is measured, not derived: |c_25,dev - c_25,ref| / c_25,ref was MEASURED_C25 (below, per plate) and is
asserted with ten times that margin."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import test_gpu_dynamics as TD
import test_gpu_modal as TM
import test_topopt_reference_host as RH
import topopt_reference as TR

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = TM.DEV
MEASURED_C25 = {"tri3": 1.978e-13, "quad4": 4.874e-14}     # on an MI355X; both loops took the same 25 x 61 decisions


@functools.lru_cache(maxsize=None)
def reference(kind):
    """(model, loss, K_e, element dofs, load, centroids, volumes, filter matrix) of a plate: built once, never modified."""
    m, lf = TM.make_model(kind), TM.make_loss("physical")
    X = m.coords.detach().double().cpu().numpy()
    conn = m.connectivity.cpu().numpy().astype(np.int64)
    node_row = TR.node_rows(m._idx_ufree.cpu().numpy(), X.shape[0])
    Ke = TR.element_matrices(X, conn, lf._mat, lf._W, "physical")
    dofs = TR.element_dofs(conn, node_row)
    b = TD.load_vector(m, lf)
    assert np.abs(b - TR.edge_load(X, m.neumann_edges.cpu().numpy(), node_row, (100e3, 0.0), lf._ci, lf._cj)).max() <= 1e-12 * np.abs(b).max()
    cen, vol = TR.geometry(X, conn)
    return m, lf, Ke, dofs, b, cen, vol, TR.filter_matrix(cen, vol, 1.5 * np.sqrt(vol.mean()))


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    reference.cache_clear()


def _fresh(kind, **kw):
    m = TM.make_model(kind, **kw)
    with torch.no_grad():
        m.u_free.zero_()
    return m


@pytest.mark.parametrize("precond", ["amg", "block_jacobi"])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_scaled_solve_against_a_sparse_direct_solve(kind, precond):
    from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver
    _, lf, Ke, dofs, b, *_ = reference(kind)
    m = _fresh(kind)
    cls = Quad4FrozenMeshSolver if kind == "quad4" else FrozenMeshSolver
    s = cls(m, lf, precond=precond, rtol=1e-10)
    n = s.n_u
    w = 10.0 ** np.random.default_rng(8).uniform(-3.0, 0.0, Ke.shape[0])
    A = TR.scaled_stiffness(Ke, dofs, w, 2 * n).tocsc()
    u_ref = spla.spsolve(A, b)
    lmin = spla.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    s.set_element_scale(torch.from_numpy(w).to(DEV))
    info = s.solve()
    u = m.u_free.detach().cpu().numpy().reshape(-1)
    r_dev, r_ref = np.linalg.norm(b - A @ u), np.linalg.norm(b - A @ u_ref)
    err = np.linalg.norm(u - u_ref)
    print(f"{kind} {precond}: {info.iterations} iterations ({info.reason}), |u - u_ref| {err:.2e} bound "
          f"{2 * (r_dev + r_ref) / lmin:.2e}, |r_dev| / |b| {r_dev / np.linalg.norm(b):.1e}")
    assert info.converged
    assert err <= 2.0 * (r_dev + r_ref) / lmin
    assert r_dev <= 10 * 1e-10 * np.linalg.norm(b)          # the recursion's residual is the true one to a small factor
    # None afterwards reproduces the unscaled solve
    K = TR.scaled_stiffness(Ke, dofs, np.ones_like(w), 2 * n).tocsc()
    u0_ref = spla.spsolve(K, b)
    l0 = spla.eigsh(K, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    s.set_element_scale(None)
    with torch.no_grad():
        m.u_free.zero_()
    info = s.solve()
    u0 = m.u_free.detach().cpu().numpy().reshape(-1)
    assert info.converged
    assert np.linalg.norm(u0 - u0_ref) <= 2.0 * (np.linalg.norm(b - K @ u0) + np.linalg.norm(b - K @ u0_ref)) / l0
    # a nonzero Dirichlet value is refused with a scale
    s.set_element_scale(torch.from_numpy(w).to(DEV))
    keep = m.u_fixed.detach().clone()
    with torch.no_grad():
        m.u_fixed.add_(0.01)
    with pytest.raises(ValueError, match="u_fixed == 0"):
        s.solve()
    with torch.no_grad():
        m.u_fixed.copy_(keep)
    for bad in (torch.zeros(Ke.shape[0], dtype=F64, device=DEV), torch.full((Ke.shape[0],), float("inf"), dtype=F64, device=DEV),
                -torch.ones(Ke.shape[0], dtype=F64, device=DEV)):
        with pytest.raises(ValueError, match="finite and > 0"):
            s.set_element_scale(bad)
    with pytest.raises(ValueError, match="shape"):
        s.set_element_scale(torch.ones(3, dtype=F64, device=DEV))


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_compliance_and_sensitivity_at_the_devices_own_displacement(kind):
    from hidenn_fem_amd.topopt import TopologyOptimizer
    _, lf, Ke, dofs, b, cen, vol, F = reference(kind)
    m = _fresh(kind)
    opt = TopologyOptimizer(m, lf, 0.4, e_min=1e-3, precond="block_jacobi", rtol=1e-10)
    rho = np.random.default_rng(12).uniform(0.2, 1.0, len(vol))
    opt.density.copy_(torch.from_numpy(rho).to(DEV))
    opt.filtered_density.copy_(opt.weights.filter(opt.density))
    rf = F @ rho
    assert np.abs(opt.filtered_density.cpu().numpy() - rf).max() <= 1e-13
    w = TR.simp(rf, 3.0, 1e-3)
    c = opt.compliance()
    u = opt.solver._u.cpu().numpy().reshape(-1)
    c_ref = float(w @ TR.element_energies(Ke, dofs, u))
    dc = opt.sensitivity().cpu().numpy()
    u = opt.solver._u.cpu().numpy().reshape(-1)
    dc_ref = F.T @ (-3.0 * rf ** 2 * (1.0 - 1e-3) * TR.element_energies(Ke, dofs, u))
    print(f"{kind}: c {c:.6e} rel {abs(c - c_ref) / c_ref:.1e}; dc rel {np.abs(dc - dc_ref).max() / np.abs(dc_ref).max():.1e}; "
          f"f^T u rel {abs(b @ u - c_ref) / c_ref:.1e}")
    assert abs(c - c_ref) <= 1e-10 * c_ref
    assert np.abs(dc - dc_ref).max() <= 1e-10 * np.abs(dc_ref).max()
    assert np.array_equal(opt.density.cpu().numpy(), rho)   # neither call updates the design


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_design_loop_against_the_reference_loop(kind):
    from hidenn_fem_amd.topopt import TopologyOptimizer
    _, lf, Ke, dofs, b, cen, vol, F = reference(kind)
    _, _, cs_ref, _, _, _ = RH.reference_loop(kind)
    m = _fresh(kind)
    x0 = m.node_coords_free.detach().clone()
    gx = torch.randn_like(m.node_coords_free)
    gu = torch.randn_like(m.u_free)
    m.node_coords_free.grad, m.u_free.grad = gx.clone(), gu.clone()
    L = RH.LOOP
    opt = TopologyOptimizer(m, lf, L["volume_fraction"], penal=L["penal"], e_min=L["e_min"], move=L["move"], n_bisect=L["n_bisect"],
                            precond="amg", rtol=1e-8)
    assert abs(opt.filter_radius - 1.5 * np.sqrt(vol.mean())) <= 1e-14
    ne = len(vol)
    target = L["volume_fraction"] * vol.sum()
    cs, its = [], []
    for k in range(L["n_iter"]):
        info = opt.step()
        rho, rf = opt.density.cpu().numpy(), opt.filtered_density.cpu().numpy()
        assert info.feasible and info.converged, (k, info)
        assert vol @ rf <= target * (1 + 4 * ne * 2.0 ** -53), k
        assert abs(info.volume - vol @ rf) <= 4 * ne * 2.0 ** -53 * target
        assert (rho >= 0).all() and (rho <= 1).all() and info.change <= L["move"] * (1 + 1e-15)
        cs.append(info.compliance)
        its.append(info.iterations)
    cs = np.array(cs)
    rel = abs(cs[-1] - cs_ref[-1]) / cs_ref[-1]
    print(f"{kind}: c_1 {cs[0]:.6e} (ref {cs_ref[0]:.6e}) c_25 {cs[-1]:.6e} (ref {cs_ref[-1]:.6e}) "
          f"|c_25,dev - c_25,ref| / c_25,ref {rel:.3e}; PCG iterations at 1, 10, 25: {its[0]}, {its[9]}, {its[24]}; max {max(its)}")
    assert (np.diff(cs) < 0).all(), cs
    assert cs[-1] <= 0.5 * cs[0]
    assert abs(cs[0] - cs_ref[0]) <= 1e-6 * cs_ref[0]       # the first compliance is a plain solve at rtol 1e-8
    assert rel <= 10 * MEASURED_C25[kind]
    # of the model only u_free moved
    assert torch.equal(m.node_coords_free.detach(), x0)
    assert torch.equal(m.node_coords_free.grad, gx) and torch.equal(m.u_free.grad, gu)


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_row_order_fp32_models_and_run_stops_on_tol(kind):
    from hidenn_fem_amd.topopt import TopologyOptimizer, minimize_compliance_
    lf = TM.make_loss("physical")
    out = {}
    for order in ("off", "hilbert"):                        # the design is by element: the storage row order must not show
        m = _fresh(kind, reorder=order)
        opt = TopologyOptimizer(m, lf, 0.4, e_min=1e-3, precond="block_jacobi")
        infos = opt.run(3, tol=0.0)
        assert len(infos) == 3
        out[order] = (np.array([i.compliance for i in infos]), opt.filtered_density.cpu().numpy())
    assert np.abs(out["off"][0] - out["hilbert"][0]).max() <= 1e-6 * out["off"][0].max()     # two solves at rtol 1e-8
    assert np.abs(out["off"][1] - out["hilbert"][1]).max() <= 1e-5
    # the same on the reordered model with AMG: its fine level reads w_elem by global element id (the Scaled instance of amg_assemble_kernel)
    m = _fresh(kind, reorder="hilbert")
    assert not torch.equal(m._idx_ufree.cpu(), _fresh(kind, reorder="off")._idx_ufree.cpu())     # the rows did move
    opt = TopologyOptimizer(m, lf, 0.4, e_min=1e-3, precond="amg")
    infos = opt.run(3, tol=0.0)
    assert all(i.converged and i.feasible for i in infos)
    assert np.abs(np.array([i.compliance for i in infos]) - out["off"][0]).max() <= 1e-6 * out["off"][0].max()
    assert np.abs(opt.filtered_density.cpu().numpy() - out["off"][1]).max() <= 1e-5
    # and the assembled K(w) of the reordered model against the reference in its own row order
    from hidenn_fem_amd.solve import assemble_stiffness
    from test_gpu_dynamics_kernels import _scipy
    X = m.coords.detach().double().cpu().numpy()
    conn = m.connectivity.cpu().numpy().astype(np.int64)
    Ke = TR.element_matrices(X, conn, lf._mat, lf._W, "physical")
    dofs = TR.element_dofs(conn, TR.node_rows(m._idx_ufree.cpu().numpy(), X.shape[0]))
    w = 10.0 ** np.random.default_rng(21).uniform(-9.0, 0.0, conn.shape[0])
    A = TR.scaled_stiffness(Ke, dofs, w, 2 * int(m.u_free.shape[0]))
    got = _scipy(assemble_stiffness(m, lf, elem_scale=torch.from_numpy(w).to(DEV)))
    assert abs(got - A).max() <= 1e-12 * abs(A).max()
    # an fp32 model: solved in fp64 from coordinates rounded to fp32 (6e-8 relative; the jittered cells are ~1/22 wide, so
    # strains move by ~1e-6 relative) and u_free rounded on write-back, which only the warm start sees
    m32 = _fresh(kind, dtype=torch.float32, reorder="off")
    opt = TopologyOptimizer(m32, TM.make_loss("physical", dtype=torch.float32), 0.4, e_min=1e-3, precond="block_jacobi")
    infos = opt.run(3, tol=0.0)
    assert m32.u_free.dtype == torch.float32 and opt.density.dtype == F64
    assert np.abs(np.array([i.compliance for i in infos]) - out["off"][0]).max() <= 1e-4 * out["off"][0].max()
    # run() stops on tol: the move limit bounds the change by 0.2, so tol = 0.5 is met by the first step
    m = _fresh(kind)
    opt = TopologyOptimizer(m, lf, 0.4, e_min=1e-3, precond="block_jacobi")
    assert len(opt.run(10, tol=0.5)) == 1
    m = _fresh(kind)
    rf, infos, c = minimize_compliance_(m, lf, 0.4, n_iter=2, tol=0.0, e_min=1e-3, precond="block_jacobi")
    assert len(infos) == 2 and c < infos[-1].compliance and rf.shape == (m.connectivity.shape[0],)
    assert torch.isfinite(m.u_free).all() and m.u_free.abs().max() > 0


@pytest.mark.parametrize("quad", [False, True])
def test_example4_prints_a_design_history(capsys, quad):
    """``python -m examples.example4 --topopt 4 --precond amg [--quad]`` on 40 x 20 nodes: one line per design iteration, the
    volume fraction held at 0.4, the compliance decreasing."""
    import examples.example4 as e4
    model, opt, infos = e4.run(nx=40, ny=20, dtype=F64, topopt=4, precond="amg", quad=quad)
    out = capsys.readouterr().out
    assert out.count("iteration ") == 4 and "INFEASIBLE" not in out and "4 design iterations" in out
    cs = [i.compliance for i in infos]
    assert all(b < a for a, b in zip(cs, cs[1:])) and all(i.feasible and i.converged for i in infos)
    total = float(opt.volumes.sum())
    assert all(abs(i.volume / total - 0.4) <= 1e-9 for i in infos)
