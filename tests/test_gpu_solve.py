"""Frozen-mesh displacement solve (hidenn_fem_amd/solve.py, csrc/cg.hip, csrc/tri3_cg.hip): the CG matrix-vector product against the
graded energy kernel, the block-Jacobi blocks and the solution against the dense oracle Hessian of the reference chain, the
minimum of the graded energy, the model contract, graph replay / halt and breakdown."""
import numpy as np
import pytest
import torch

from conftest import tri_case_forces, tri_mesh_dict

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")


def _golden_model(g, case, u_fixed=0.0, conv="reference"):
    from test_gpu_parity import tri_model_from_golden
    m = tri_model_from_golden(g, case, DEV)
    if not isinstance(u_fixed, float):                                 # nonzero Dirichlet values
        m.u_fixed = torch.as_tensor(u_fixed, dtype=F64, device=DEV)
    m.grad_convention = conv
    return m


def _loss(g, case):
    from hidenn_fem_amd.loss import EnergyLoss2D
    go, go1 = (int(v) for v in g[case + "/gauss_order"])
    return EnergyLoss2D(E=10e9, nu=0.3, gauss_order=go, gauss_order_1d=go1, device=DEV, dtype=F64), go, go1


def _dev_forces(case):
    b, t = tri_case_forces(case)
    bd = (lambda x: b(x.cpu().double()).to(x.device)) if b else None
    td = (lambda x: t(x.cpu().double()).to(x.device)) if t else None
    return b, t, bd, td


_ORACLE = {}


def _oracle(g, case, conv, u_fixed=None):
    key = (case, conv, None if u_fixed is None else tuple(u_fixed))
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_dense(g, case, conv, u_fixed)
    return _ORACLE[key]


def _oracle_dense(g, case, conv, u_fixed=None):
    """Dense K_ff (fp64, CPU, autograd Hessian of oracle.ref_chain.total_energy w.r.t. u_free) and f = -dE/du at u_free = 0."""
    from oracle.ref_chain import total_energy
    mesh, xf, uf = tri_mesh_dict(g, case)
    if u_fixed is not None:
        mesh["u_fixed"] = torch.as_tensor(u_fixed, dtype=F64)
    go, go1 = (int(v) for v in g[case + "/gauss_order"])
    b, t = tri_case_forces(case)
    fn = lambda u: total_energy(xf, u, mesh, gauss_order=go, gauss_order_1d=go1, b_force=b, t_force=t, convention=conv)
    n = uf.numel()
    H = torch.autograd.functional.hessian(fn, torch.zeros_like(uf)).reshape(n, n)
    u0 = torch.zeros_like(uf).requires_grad_(True)
    f = -torch.autograd.grad(fn(u0), u0)[0].reshape(n)
    return H, f, uf.shape


def _solve_cases(g):
    return [c for c in g.cases() if c != "mini_example4" and bool(g[c + "/dirichlet_mask"].any())]


# ---------------------------------------------------------------- 1. apply vs the graded kernel
def _check_apply(m, lf):
    from hidenn_fem_amd.solve import FrozenMeshSolver
    torch.manual_seed(1)
    s = FrozenMeshSolver(m, lf)
    p = torch.randn(m.u_free.shape, dtype=F64, device=DEV) * 1e-4
    q, pq = s.apply(p)
    with torch.no_grad():
        m.u_free.copy_(p)
    m.zero_grad(set_to_none=True)
    e = lf.domain_energy(m)                 # no forces, edges off, u_fixed = 0: E = 1/2 p^T K p, dE/du = K p
    e.backward()
    want = m.u_free.grad
    scale = want.abs().max().item()
    assert (q - want).abs().max().item() <= 1e-12 * scale
    assert abs(pq.item() - 2.0 * e.item()) <= 1e-12 * abs(2.0 * e.item())


@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_apply_matches_the_graded_energy_kernel_on_the_golden_cases(g_tri, conv):
    for case in g_tri.cases():
        lf, _, _ = _loss(g_tri, case)
        _check_apply(_golden_model(g_tri, case, conv=conv), lf)


@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_apply_matches_the_graded_energy_kernel_on_a_large_unstructured_mesh(conv):
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import unstructured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = unstructured_tri_mesh(52000, dtype=F64)
    assert conn.shape[0] > 90000
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(DEV)
    m.grad_convention = conv
    _check_apply(m, EnergyLoss2D(device=DEV, dtype=F64))


# ---------------------------------------------------------------- 2. block Jacobi vs the dense oracle
@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_block_jacobi_blocks_match_the_oracle_hessian(g_tri, conv):
    from hidenn_fem_amd.solve import FrozenMeshSolver
    for case in ("order4", "flipped", "permuted_random_diag"):
        H, _, shp = _oracle(g_tri, case, conv)
        n = shp[0]
        Hb = H.reshape(n, 2, n, 2)
        idx = torch.arange(n)
        blk = Hb[idx, :, idx, :]                                       # [n, 2, 2]
        want = torch.stack([blk[:, 0, 0], 0.5 * (blk[:, 0, 1] + blk[:, 1, 0]), blk[:, 1, 1]], dim=1)
        lf, _, _ = _loss(g_tri, case)
        s = FrozenMeshSolver(_golden_model(g_tri, case, conv=conv), lf)
        s.refresh()
        got = s.diag.cpu()
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), case


# ---------------------------------------------------------------- 3. solution vs a dense solve
@pytest.mark.parametrize("conv", ["reference", "physical"])
@pytest.mark.parametrize("precond", ["block_jacobi", "none"])
def test_solution_matches_a_dense_solve_of_the_oracle_system(g_tri, conv, precond):
    from hidenn_fem_amd.solve import FrozenMeshSolver
    cases = [(c, None) for c in _solve_cases(g_tri)] + [("order4_body", [3.0e-5, -2.0e-5])]
    assert any(c == "traction_fn" for c, _ in cases) and any(c.endswith("_body") for c, _ in cases)
    for case, ufix in cases:
        H, f, shp = _oracle(g_tri, case, conv, u_fixed=ufix)
        ustar = torch.linalg.solve(H, f).reshape(shp)
        lf, _, _ = _loss(g_tri, case)
        _, _, bd, td = _dev_forces(case)
        m = _golden_model(g_tri, case, u_fixed=0.0 if ufix is None else ufix, conv=conv)
        info = FrozenMeshSolver(m, lf, b_force=bd, t_force=td, precond=precond, rtol=1e-12).solve()
        assert info.converged and info.reason == "rtol", (case, info)
        err = (m.u_free.detach().cpu() - ustar).abs().max().item()
        assert err <= 1e-9 * ustar.abs().max().item(), (case, ufix, err)
        assert abs(info.rhs_norm - f.norm().item()) <= 1e-10 * f.norm().item()


# ---------------------------------------------------------------- 4. minimum of the graded energy
def _plate(nx, ny):
    from hidenn_fem_amd.mesh import generate_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nodes, conn, geom, bc, mn, edges = generate_mesh(2.0, 1.0, [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)],
                                                     {"up": 0, "down": 0, "right": 2, "left": 1}, nx, ny)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nodes.double(), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                    neumann_edges=edges).to(DEV)


@pytest.mark.parametrize("which", ["mini_example4", "plate_1e5"])
def test_solve_reaches_the_minimum_of_the_graded_energy(g_tri, which):
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.optim import FusedLBFGS
    from hidenn_fem_amd.solve import solve_displacement_
    import copy
    if which == "mini_example4":
        m = _golden_model(g_tri, which)
    else:
        m = _plate(330, 165)
        assert m.Nelems > 90000
    lf = EnergyLoss2D(device=DEV, dtype=F64)
    m_lbfgs = copy.deepcopy(m)
    info = solve_displacement_(m, lf, rtol=1e-10)
    assert info.converged, info
    e_solve = lf.value_and_grad_(m).item()
    gnorm = m.u_free.grad.norm().item()
    assert gnorm <= 1e-9 * info.rhs_norm, (gnorm, info)
    opt = FusedLBFGS([m_lbfgs.u_free])
    for _ in range(30):
        opt.step(lambda: lf.value_and_grad_(m_lbfgs))
    e_lbfgs = lf.value_and_grad_(m_lbfgs).item()
    assert e_solve <= e_lbfgs + 1e-12 * abs(e_lbfgs), (e_solve, e_lbfgs)


# ---------------------------------------------------------------- 5. contract
def test_model_state_other_than_u_free_is_untouched(g_tri):
    from hidenn_fem_amd.solve import solve_displacement_
    case = "traction_fn"
    lf, _, _ = _loss(g_tri, case)
    _, _, bd, td = _dev_forces(case)
    m = _golden_model(g_tri, case, u_fixed=[1e-5, 2e-5])
    x0, xfix0, ufix0 = m.node_coords_free.detach().clone(), m.node_coords_fixed.clone(), m.u_fixed.clone()
    ufull_dir0 = m.u_full.detach()[m.dirichlet_mask].clone()
    assert m.node_coords_free.grad is None and m.u_free.grad is None
    info = solve_displacement_(m, lf, b_force=bd, t_force=td)
    assert info.converged
    assert torch.equal(m.node_coords_free.detach(), x0) and torch.equal(m.node_coords_fixed, xfix0)
    assert torch.equal(m.u_fixed, ufix0) and torch.equal(m.u_full.detach()[m.dirichlet_mask], ufull_dir0)
    assert m.node_coords_free.grad is None and m.u_free.grad is None


def _structured(reorder, dtype=F64, nx=101, ny=61):
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(nx, ny, jitter=0.25, seed=3, dtype=F64)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nc.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                    neumann_edges=edges, reorder=reorder).to(DEV)


def test_tile_major_rows_give_the_caller_order_solution_of_reorder_off():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import solve_displacement_
    lf = EnergyLoss2D(device=DEV, dtype=F64)
    ma, mo = _structured("auto"), _structured("off")
    assert ma.row_order == "tile" and mo.row_order == "as given"
    ia = solve_displacement_(ma, lf, rtol=1e-12)
    io = solve_displacement_(mo, lf, rtol=1e-12)
    assert ia.converged and io.converged
    ua, uo = ma.to_caller_order(ma.u_free.detach(), "u"), mo.u_free.detach()
    assert (ua - uo).abs().max().item() <= 1e-12 * uo.abs().max().item()


def test_fp32_model_is_the_fp64_solve_rounded_once():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import solve_displacement_
    m32 = _structured("auto", dtype=torch.float32, nx=61, ny=41)
    m64 = _structured("auto", dtype=torch.float32, nx=61, ny=41).double()
    i32 = solve_displacement_(m32, EnergyLoss2D(device=DEV, dtype=torch.float32), rtol=1e-12)
    i64 = solve_displacement_(m64, EnergyLoss2D(device=DEV, dtype=F64), rtol=1e-12)
    assert i32.converged and i64.converged and m32.u_free.dtype == torch.float32
    want = m64.u_free.detach().float()
    assert (m32.u_free.detach() - want).abs().max().item() <= 2e-7 * want.abs().max().item()


def test_solve_refreshes_by_itself_after_the_coordinates_moved():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import FrozenMeshSolver
    lf = EnergyLoss2D(device=DEV, dtype=F64)
    m = _structured("auto", nx=61, ny=41)
    s = FrozenMeshSolver(m, lf, rtol=1e-12)
    assert s.solve().converged
    with torch.no_grad():                                              # an r-adaptive coordinate step, in place
        torch.manual_seed(7)
        m.node_coords_free.add_(2e-3 * torch.randn_like(m.node_coords_free))
    u_start = m.u_free.detach().clone()
    assert s.solve().converged
    got = m.u_free.detach().clone()
    with torch.no_grad():
        m.u_free.copy_(u_start)
    assert FrozenMeshSolver(m, lf, rtol=1e-12).solve().converged
    want = m.u_free.detach()
    assert (got - want).abs().max().item() <= 1e-9 * want.abs().max().item()


# ---------------------------------------------------------------- 6. graph replay / halt
def test_iterations_per_graph_do_not_change_the_result_and_replays_after_the_halt_do_nothing():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import FrozenMeshSolver
    lf = EnergyLoss2D(device=DEV, dtype=F64)
    out = {}
    for k in (1, 8):
        m = _structured("auto", nx=61, ny=41)
        s = FrozenMeshSolver(m, lf, rtol=1e-10, iters_per_graph=k)
        info = s.solve()
        assert info.converged
        out[k] = (info, m.u_free.detach().clone(), s)
    (i1, u1, _), (i8, u8, s8) = out[1], out[8]
    assert i1.iterations == i8.iterations
    assert (u1 - u8).abs().max().item() <= 1e-12 * u8.abs().max().item()
    st0, u0 = s8._read_status(), s8._u.clone()
    for _ in range(3):
        s8._replay()
    assert s8._read_status() == st0 and torch.equal(s8._u, u0)


# ---------------------------------------------------------------- 7. breakdown
def test_singular_system_ends_unconverged_with_finite_displacements():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.solve import solve_displacement_
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(31, 21, jitter=0.2, seed=2, dtype=F64)
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=None, u_fixed=None, neumann_edges=edges).to(DEV)
    assert m.u_free.shape[0] == nc.shape[0]                            # no Dirichlet rows: K has rigid-body modes
    info = solve_displacement_(m, EnergyLoss2D(device=DEV, dtype=F64), rtol=1e-10, max_iter=400, iters_per_graph=8)
    assert not info.converged and info.reason in ("breakdown", "max_iter"), info
    assert torch.isfinite(m.u_free).all()
