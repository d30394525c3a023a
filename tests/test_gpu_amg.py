"""Smoothed-aggregation AMG preconditioner of the frozen-mesh solve (hidenn_fem_amd/solve.py precond="amg",
csrc/tri3_amg.hip): the assembled K_ff against the dense oracle Hessian and the matrix-free apply, every level's P and A_c
against a numpy restatement of the numeric setup, the V-cycle's symmetry and determinism, solutions against the dense oracle
solve and block Jacobi, iteration counts, the solver contract, the numeric-only refresh and the r-adaptive loop."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from cg_reference import _bsr, _mgs, _power
from test_gpu_solve import _dev_forces, _golden_model, _loss, _oracle, _plate, _solve_cases, _structured

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")


def _unstructured(n=52000, reorder="auto"):
    from hidenn_fem_amd.mesh import unstructured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = unstructured_tri_mesh(n, dtype=F64)
    torch.manual_seed(0)
    return PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges,
                                    reorder=reorder).to(DEV)


def _lf():
    from hidenn_fem_amd.loss import EnergyLoss2D
    return EnergyLoss2D(device=DEV, dtype=F64)


# ---------------------------------------------------------------- 1. assembly vs the dense oracle Hessian
@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_assembled_stiffness_equals_the_oracle_hessian(g_tri, conv):
    from hidenn_fem_amd.solve import assemble_stiffness
    for case in _solve_cases(g_tri):
        H, _, shp = _oracle(g_tri, case, conv)
        lf, _, _ = _loss(g_tri, case)
        K = assemble_stiffness(_golden_model(g_tri, case, conv=conv), lf)
        assert K.layout == torch.sparse_bsr and K.dtype == F64 and K.values().shape[1:] == (2, 2)
        got = K.to_dense().cpu()
        assert got.shape == H.shape
        assert (got - H).abs().max().item() <= 1e-12 * H.abs().max().item(), case


# ---------------------------------------------------------------- 2. assembled K p vs the matrix-free apply
@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_assembled_kp_equals_the_matrix_free_apply_on_tile_major_delaunay_rows(conv):
    from hidenn_fem_amd.solve import FrozenMeshSolver, assemble_stiffness
    m = _unstructured()
    assert m.row_order == "tile" and m.Nelems > 90000
    m.grad_convention = conv
    lf = _lf()
    K = assemble_stiffness(m, lf)
    s = FrozenMeshSolver(m, lf)
    torch.manual_seed(3)
    p = torch.randn(m.u_free.shape, dtype=F64, device=DEV)
    q, _ = s.apply(p)
    kp = (K @ p.reshape(-1, 1)).reshape(-1, 2)
    assert (kp - q).abs().max().item() <= 1e-12 * q.abs().max().item()


# ---------------------------------------------------------------- 3. the numeric setup vs a numpy restatement
@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_every_level_matches_a_numpy_restatement_and_coarse_operators_are_symmetric(conv):
    from hidenn_fem_amd.solve import FrozenMeshSolver
    m = _structured("auto", nx=121, ny=61)
    m.grad_convention = conv
    s = FrozenMeshSolver(m, _lf(), precond="amg")
    s.refresh()
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
            Q, R = _mgs(ns[mem].reshape(-1, 3))
            T[mem] = Q.reshape(len(mem), bs, 3)
            Rn[J] = R
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


# ---------------------------------------------------------------- 4. the V-cycle is SPD and deterministic
def test_vcycle_is_symmetric_positive_definite_and_bit_reproducible():
    from hidenn_fem_amd.solve import FrozenMeshSolver
    m = _unstructured(20000)
    lf = _lf()
    s = FrozenMeshSolver(m, lf, precond="amg")
    assert s.amg["levels"] >= 3
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(3):
        x = torch.randn(m.u_free.shape, dtype=F64, device=DEV, generator=g)
        y = torch.randn(m.u_free.shape, dtype=F64, device=DEV, generator=g)
        Mx, My = s.precondition(x), s.precondition(y)
        lhs, rhs = (x * My).sum().item(), (y * Mx).sum().item()
        assert abs(lhs - rhs) <= 1e-10 * x.norm().item() * My.norm().item()
        assert (x * Mx).sum().item() > 0.0
    z1 = s.precondition(x)
    z2 = s.precondition(x)
    s2 = FrozenMeshSolver(m, lf, precond="amg")
    z3 = s2.precondition(x)
    assert torch.equal(z1, z2) and torch.equal(z1, z3)
    assert torch.equal(s._amg.coarse_inv, s2._amg.coarse_inv)


# ---------------------------------------------------------------- 5. solutions
@pytest.mark.parametrize("conv", ["reference", "physical"])
def test_amg_solution_matches_a_dense_solve_of_the_oracle_system(g_tri, conv):
    from hidenn_fem_amd.solve import FrozenMeshSolver
    cases = [(c, None) for c in _solve_cases(g_tri)] + [("order4_body", [3.0e-5, -2.0e-5])]
    for case, ufix in cases:
        H, f, shp = _oracle(g_tri, case, conv, u_fixed=ufix)
        ustar = torch.linalg.solve(H, f).reshape(shp)
        lf, _, _ = _loss(g_tri, case)
        _, _, bd, td = _dev_forces(case)
        m = _golden_model(g_tri, case, u_fixed=0.0 if ufix is None else ufix, conv=conv)
        info = FrozenMeshSolver(m, lf, b_force=bd, t_force=td, precond="amg", rtol=1e-12).solve()
        assert info.converged and info.reason == "rtol", (case, info)
        err = (m.u_free.detach().cpu() - ustar).abs().max().item()
        assert err <= 1e-9 * ustar.abs().max().item(), (case, ufix, err)


def _iters(m, precond, rtol=1e-8):
    from hidenn_fem_amd.solve import FrozenMeshSolver
    with torch.no_grad():
        m.u_free.zero_()
    info = FrozenMeshSolver(m, _lf(), precond=precond, rtol=rtol).solve()
    assert info.converged, (precond, info)
    return info.iterations, m.u_free.detach().clone()


def test_amg_matches_block_jacobi_on_a_1e5_plate():
    m = _plate(330, 165)
    assert m.Nelems > 90000
    ib, ub = _iters(m, "block_jacobi", 1e-10)
    ia, ua = _iters(m, "amg", 1e-10)
    assert (ua - ub).abs().max().item() <= 1e-7 * ub.abs().max().item()
    assert ia * 10 <= ib, (ia, ib)


# ---------------------------------------------------------------- 6. iteration counts
def test_amg_needs_a_tenth_of_block_jacobi_iterations_and_scales():
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    out = {}
    for name, m in (("structured", _structured("auto", nx=351, ny=176)), ("delaunay", _unstructured(32000))):
        ib, _ = _iters(m, "block_jacobi")
        ia, _ = _iters(m, "amg")
        out[name] = (ia, ib)
        assert ia * 10 <= ib, (name, ia, ib)
    counts = {}
    for nx, ny in ((251, 126), (1001, 501)):
        nc, conn, geom, bc, mn, edges = structured_tri_mesh(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
        torch.manual_seed(0)
        m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(DEV)
        counts[m.Nelems] = _iters(m, "amg")[0]
        del m
    (n0, i0), (n1, i1) = sorted(counts.items())
    assert n0 < 7e4 and n1 >= 1e6
    assert i1 <= 1.5 * i0, (counts, out)


# ---------------------------------------------------------------- 7. contract
def test_amg_contract_fp32_row_order_graph_halt_and_untouched_state():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.solve import FrozenMeshSolver, solve_displacement_
    # fp32 model = the fp64 solve rounded once
    m32 = _structured("auto", dtype=torch.float32, nx=61, ny=41)
    m64 = _structured("auto", dtype=torch.float32, nx=61, ny=41).double()
    assert solve_displacement_(m32, EnergyLoss2D(device=DEV, dtype=torch.float32), precond="amg", rtol=1e-12).converged
    assert solve_displacement_(m64, _lf(), precond="amg", rtol=1e-12).converged
    want = m64.u_free.detach().float()
    assert (m32.u_free.detach() - want).abs().max().item() <= 2e-7 * want.abs().max().item()
    # tile-major rows = reorder off, in caller order
    ma, mo = _structured("auto"), _structured("off")
    assert solve_displacement_(ma, _lf(), precond="amg", rtol=1e-12).converged
    assert solve_displacement_(mo, _lf(), precond="amg", rtol=1e-12).converged
    ua, uo = ma.to_caller_order(ma.u_free.detach(), "u"), mo.u_free.detach()
    assert (ua - uo).abs().max().item() <= 1e-12 * uo.abs().max().item()
    # iters_per_graph does not change the result; replays after the halt do nothing; state untouched
    res = {}
    for k in (1, 8):
        m = _structured("auto", nx=61, ny=41)
        x0, xfix0 = m.node_coords_free.detach().clone(), m.node_coords_fixed.clone()
        udir0 = m.u_full.detach()[m.dirichlet_mask].clone()
        s = FrozenMeshSolver(m, _lf(), precond="amg", rtol=1e-10, iters_per_graph=k)
        info = s.solve()
        assert info.converged
        assert torch.equal(m.node_coords_free.detach(), x0) and torch.equal(m.node_coords_fixed, xfix0)
        assert torch.equal(m.u_full.detach()[m.dirichlet_mask], udir0)
        assert m.node_coords_free.grad is None and m.u_free.grad is None
        res[k] = (info, m.u_free.detach().clone(), s)
    (i1, u1, _), (i8, u8, s8) = res[1], res[8]
    assert i1.iterations == i8.iterations          # the apply's LDS atomics leave run-to-run last bits
    assert (u1 - u8).abs().max().item() <= 1e-12 * u8.abs().max().item()
    st0, u0 = s8._read_status(), s8._u.clone()
    for _ in range(3):
        s8._replay()
    assert s8._read_status() == st0 and torch.equal(s8._u, u0)


# ---------------------------------------------------------------- 8. a coordinate change redoes the numeric setup only
def test_coordinate_change_redoes_only_the_numeric_setup():
    from hidenn_fem_amd.solve import FrozenMeshSolver, amg_host
    lf = _lf()
    m = _structured("auto", nx=61, ny=41)
    s = FrozenMeshSolver(m, lf, precond="amg", rtol=1e-12)
    host = amg_host(m)
    assert s.solve().converged and s.amg["numeric_setups"] == 1
    with torch.no_grad():
        torch.manual_seed(7)
        m.node_coords_free.add_(2e-3 * torch.randn_like(m.node_coords_free))
    u_start = m.u_free.detach().clone()
    assert s.solve().converged
    assert s.amg["numeric_setups"] == 2 and amg_host(m) is host and s._amg.host is host
    got = m.u_free.detach().clone()
    with torch.no_grad():
        m.u_free.copy_(u_start)
    assert FrozenMeshSolver(m, lf, precond="amg", rtol=1e-12).solve().converged
    want = m.u_free.detach()
    assert (got - want).abs().max().item() <= 1e-9 * want.abs().max().item()


# ---------------------------------------------------------------- 9. r-adaptive loop
def test_r_adaptive_run_with_amg_follows_block_jacobi():
    from hidenn_fem_amd.radapt import RAdaptiveSolver, mesh_quality
    from test_gpu_radapt import _plate as _radapt_plate
    out = {}
    for pc in ("block_jacobi", "amg"):
        m = _radapt_plate()
        info = RAdaptiveSolver(m, _lf(), cg_rtol=1e-10, max_outer=5, cg_precond=pc).run()
        assert mesh_quality(m).n_inverted == 0
        out[pc] = info.energy
    eb, ea = out["block_jacobi"], out["amg"]
    assert len(ea) == len(eb) == 6
    for a, b in zip(ea, eb):
        assert abs(a - b) <= 1e-8 * abs(b), (ea, eb)
