"""Elastoplastic load paths on the device (hidenn_fem_amd.plasticity.ElastoplasticSolver: csrc/tri3_j2.hip, csrc/cg.hip) against
the numpy statement (tests/plasticity_reference.py; its paths are pinned by tests/test_plasticity_reference_host.py).

The two cantilevers: structured_tri_mesh on [0, 2] x [0, 1], left edge clamped, a vertical traction of 2e4 on the right edge
(the callable is (0, 1e4): the engine's edge rule weighs it by 2, plasticity_reference.EDGE_C), E = 10e9, nu = 0.3, H = 5e8,
23 x 17 nodes with sigma_y = 6e4 and 17 x 9 with sigma_y = 1e5, loads [0.25, 0.5, 0.75, 1, 0.6, 0.2, -0.2, -0.6].  The loss is
built with gauss_order=1, whose weights sum to the reference triangle's area (W = 1/2: A_e is the element's area, as in the
buckling analysis); the default order 4 of the project this one was modelled on sums to 1/4.

Every device step is compared with a reference step taken from the device's own committed state and start vector, so history
errors do not accumulate: |u_dev - u_ref|_2 <= 2 (|R_dev| + |R_ref|) / lambda_min(K_T,ff at the reference's converged state),
both residuals evaluated by the reference, rtol = 1e-10.  Worst ratio measured on the MI355X: 7.3e-5 (23x17), 1.4e-3 (17x9).
The whole path end to end against the reference's own path: max|u_dev - u_ref| / max|u_ref| measured 4.6e-13 (23x17) and
1.9e-13 (17x9) over all steps; asserted with ten times margin, E2E_TOL = 4.6e-12 (the issue caps it at 1e-6)."""
import numpy as np
import pytest
import torch

import plasticity_reference as P

F64 = torch.float64
pytestmark = pytest.mark.gpu
E2E_TOL = 4.6e-12
_cache = {}


def dev():
    return torch.device("cuda:0")


def traction(x):
    return torch.stack([torch.full_like(x[:, 0], P.TRACTION[0]), torch.full_like(x[:, 0], P.TRACTION[1])], dim=1)


def make(name, precond="block_jacobi", dtype=F64, **kw):
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.plasticity import ElastoplasticSolver, J2PlasticityLoss2D
    (coords, conn, geom, bc, _, edges), prob = P.cantilever(name)
    m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                 neumann_edges=edges).to(dev())
    with torch.no_grad():
        m.u_free.zero_()
    mat = prob.mat
    lf = J2PlasticityLoss2D(E=mat.E, nu=mat.nu, sigma_y=mat.sigma_y, hardening=mat.H, gauss_order=1, device=dev(), dtype=dtype)
    kw.setdefault("rtol", 1e-10)
    return m, ElastoplasticSolver(m, lf, t_force=traction, precond=precond, **kw), prob


def to_ref(m, rows):
    return m.to_caller_order(rows.detach(), "u").cpu().double().numpy()


def state_np(s, trial=False):
    ep, al = s.state(trial)
    return ep.cpu().numpy(), al.cpu().numpy()


def compare_step(prob, u0, ep, al, load, u_dev):
    """-> (ratio |u_dev - u_ref| / bound, the reference step)"""
    ref = P.step(prob, u0, ep, al, load, rtol=1e-10)
    assert ref.converged
    r_dev = np.linalg.norm(prob.energy(u_dev, ep, al, load)[1])
    r_ref = np.linalg.norm(prob.energy(ref.u, ep, al, load)[1])
    lam_min = np.linalg.eigvalsh(prob.tangent(ref.u, ep, al, load))[0]
    assert lam_min > 0
    bound = 2 * (r_dev + r_ref) / lam_min
    return np.linalg.norm(u_dev - ref.u) / bound, ref


def device_path(name, precond):
    """The whole path on the device, each step checked against a reference step from the device's own state; cached."""
    key = (name, precond)
    if key in _cache:
        return _cache[key]
    m, s, prob = make(name, precond)
    ref_path = P.cantilever_path(name)
    u0 = np.zeros((prob.n, 2))
    ep, al = prob.virgin()
    infos, us, ratios, e2e, fracs = [], [], [], [], []
    for k, load in enumerate(P.LOADS):
        info = s.solve(load)
        u_dev = to_ref(m, m.u_free)
        ratio, ref = compare_step(prob, u0, ep, al, load, u_dev)
        # state(), stress(), von_mises(): the return map at the device's own u, by the reference
        r = prob.point(u_dev, ep, al, load)
        ep_d, al_d = state_np(s)
        sig_d = s.stress().cpu().numpy()
        errs = (np.abs(ep_d - r["ep"]).max() / max(np.abs(r["ep"]).max(), 1e-300), np.abs(al_d - r["al"]).max() / max(r["al"].max(), 1e-300),
                np.abs(sig_d - r["sig"]).max() / np.abs(r["sig"]).max(),
                np.abs(s.von_mises().cpu().numpy() - P.von_mises(r["sig"])).max() / np.abs(r["sig"]).max())
        e2e.append(np.abs(u_dev - ref_path[k].u).max() / np.abs(ref_path[k].u).max())
        print(name, precond, "load", load, "newton", info.newton_iterations, "cg", info.cg_iterations, info.reason, "ratio",
              f"{ratio:.3e}", "state/stress errors", ["%.1e" % e for e in errs], "plastic", s.plastic_fraction, r["plastic"].mean(),
              "end to end", f"{e2e[-1]:.3e}")
        assert info.converged
        assert all(e <= 1e-10 for e in errs)
        assert abs(s.plastic_fraction - r["plastic"].mean()) <= 2.0 / prob.mesh.ne
        infos.append(info)
        us.append(u_dev)
        ratios.append(ratio)
        fracs.append(s.plastic_fraction)
        u0, ep, al = u_dev, ep_d, al_d
    _cache[key] = dict(m=m, s=s, prob=prob, infos=infos, us=us, ratios=ratios, e2e=e2e, fracs=fracs)
    return _cache[key]


# ---------------------------------------------------------------- 1. the two paths
@pytest.mark.parametrize("name", list(P.CANTILEVERS))
def test_every_step_against_a_reference_step_from_the_devices_own_state(name):
    d = device_path(name, "block_jacobi")
    print(name, "worst ratio", max(d["ratios"]))
    assert max(d["ratios"]) <= 1.0
    e = [i.energy for info in d["infos"] for i in [info]]
    assert all(np.isfinite(e))
    for info in d["infos"]:                                            # the line search never lets the energy rise
        en = [h["energy"] for h in info.history] + [info.energy]
        assert all(b <= a + 4 * P.EPS * abs(a) for a, b in zip(en, en[1:]))


@pytest.mark.parametrize("name", list(P.CANTILEVERS))
def test_the_whole_path_end_to_end(name):
    d = device_path(name, "block_jacobi")
    ref = P.cantilever_path(name)
    print(name, "end to end max|u_dev - u_ref| / max|u_ref| per step", ["%.2e" % e for e in d["e2e"]])
    assert max(d["e2e"]) <= E2E_TOL
    fr = [r.plastic.mean() for r in ref]
    assert all(abs(a - b) <= 2.0 / d["prob"].mesh.ne for a, b in zip(d["fracs"], fr))
    ep_d, al_d = state_np(d["s"])
    assert np.abs(al_d - ref[-1].al).max() <= 1e-6 * ref[-1].al.max()
    assert np.abs(ep_d - ref[-1].ep).max() <= 1e-6 * np.abs(ref[-1].ep).max()


def test_amg_and_block_jacobi_reach_the_same_solution_and_amg_takes_fewer_iterations():
    name = "17x9"
    a, b = device_path(name, "amg"), device_path(name, "block_jacobi")
    assert max(a["ratios"]) <= 1.0
    cg_a, cg_b = sum(i.cg_iterations for i in a["infos"]), sum(i.cg_iterations for i in b["infos"])
    diff = max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a["us"], b["us"]))
    print("CG iterations amg", cg_a, "block Jacobi", cg_b, "max difference", diff)
    assert cg_a < cg_b
    assert diff <= 2 * E2E_TOL                                         # each lies within E2E_TOL of its own reference path


# ---------------------------------------------------------------- 2. displacement control
def ramp_problem():
    """The 17 x 9 plate, left AND right edge Dirichlet: the right edge is moved by (0, 8e-5) at load 1; no tractions."""
    (coords, conn, geom, _, _, _), base = P.cantilever("17x9")
    x = coords.numpy()
    bc = (x[:, 0] < 1e-12) | (x[:, 0] > 2.0 - 1e-12)
    ufix = np.zeros((int(bc.sum()), 2))
    ufix[x[bc][:, 0] > 1.0, 1] = 8e-5
    return coords, conn, geom, bc, ufix, P.Problem(x, conn.numpy(), bc, base.mat, 0.5, ufix, None)


def test_displacement_controlled_ramp_scales_u_fixed_by_the_load():
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.plasticity import ElastoplasticSolver, J2PlasticityLoss2D
    coords, conn, geom, bc, ufix, prob = ramp_problem()
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=torch.as_tensor(bc),
                                 u_fixed=torch.as_tensor(ufix)).to(dev())
    with torch.no_grad():
        m.u_free.zero_()
    mat = prob.mat
    s = ElastoplasticSolver(m, J2PlasticityLoss2D(E=mat.E, nu=mat.nu, sigma_y=mat.sigma_y, hardening=mat.H, gauss_order=1, device=dev(), dtype=F64),
                            rtol=1e-10)
    fixed0 = m.u_fixed.detach().clone()
    u0, (ep, al) = np.zeros((prob.n, 2)), prob.virgin()
    fracs = []
    for load in (0.5, 1.0, 0.4):
        info = s.solve(load)
        u_dev = to_ref(m, m.u_free)
        ratio, ref = compare_step(prob, u0, ep, al, load, u_dev)
        print("ramp load", load, info.newton_iterations, info.cg_iterations, "ratio", ratio, "plastic", s.plastic_fraction)
        assert info.converged and ratio <= 1.0
        fracs.append(ref.plastic.mean())
        u0 = u_dev
        ep, al = state_np(s)
    assert 0.1 <= fracs[1] <= 0.9 and fracs[2] <= 0.01                 # conditions on the reference: yields, then unloads
    assert torch.equal(m.u_fixed.detach(), fixed0)                     # the model's Dirichlet values are not written
    assert torch.allclose(s._ufix, 0.4 * s._ufix0)


# ---------------------------------------------------------------- 3. contract
def test_commit_false_reset_and_function_form():
    from hidenn_fem_amd.plasticity import elastoplastic_solve_
    name = "17x9"
    m, s, prob = make(name)
    s.run(P.LOADS[:3])
    ep0, al0 = s.state()
    u_keep = m.u_free.detach().clone()
    assert al0.max().item() > 0
    a = s.solve(1.0, commit=False)
    ep1, al1 = s.state()
    assert torch.equal(ep0, ep1) and torch.equal(al0, al1)             # untouched
    tr = s.state(trial=True)[1]
    assert tr.max().item() > al0.max().item()                          # the trial state moved on
    u_a = m.u_free.detach().clone()
    with torch.no_grad():
        m.u_free.copy_(u_keep)
    b = s.solve(1.0)                                                   # the same step again, now committed
    assert a.newton_iterations == b.newton_iterations
    assert ((m.u_free.detach() - u_a).abs().max() / u_a.abs().max()).item() <= 1e-9
    assert torch.equal(s.state()[1], s.state(trial=True)[1])
    # reset: the virgin state; the first step again gives the first step's result
    first = device_path(name, "block_jacobi")["us"][0]
    s.reset()
    assert s.state()[1].abs().max().item() == 0 and s.state()[0].abs().max().item() == 0
    with torch.no_grad():
        m.u_free.zero_()
    s.solve(P.LOADS[0])
    assert np.abs(to_ref(m, m.u_free) - first).max() <= 1e-9 * np.abs(first).max()
    # the function form runs the same path
    m2, _, _ = make(name)
    infos = elastoplastic_solve_(m2, s.loss_fn, P.LOADS[:2], t_force=traction, rtol=1e-10)
    assert len(infos) == 2 and all(i.converged for i in infos)
    want = device_path(name, "block_jacobi")["us"][1]
    assert np.abs(to_ref(m2, m2.u_free) - want).max() <= 1e-9 * np.abs(want).max()


def test_row_order_and_an_fp32_model():
    """state(), stress() are in the model's element order and u in its row order: a model that stores its rows tile-major and one
    that stores them as given give the same path; an fp32 model follows the fp64 one to its rounding."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.plasticity import ElastoplasticSolver, J2PlasticityLoss2D
    name = "17x9"
    (coords, conn, geom, bc, _, edges), prob = P.cantilever(name)
    base = device_path(name, "block_jacobi")
    assert base["m"].row_order == "as given"
    mat = prob.mat
    lf = J2PlasticityLoss2D(E=mat.E, nu=mat.nu, sigma_y=mat.sigma_y, hardening=mat.H, gauss_order=1, device=dev(), dtype=F64)
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges,
                                 reorder="tile").to(dev())
    assert m.row_order == "tile"
    with torch.no_grad():
        m.u_free.zero_()
    s = ElastoplasticSolver(m, lf, t_force=traction, rtol=1e-10)
    s.run(P.LOADS[:4])
    u = to_ref(m, m.u_free)
    assert np.abs(u - base["us"][3]).max() <= 1e-9 * np.abs(u).max()
    ref = P.cantilever_path(name)[3]
    assert np.abs(s.state()[1].cpu().numpy() - ref.al).max() <= 1e-6 * ref.al.max()
    m32, s32, _ = make(name, dtype=torch.float32)
    s32.run(P.LOADS[:4])
    assert m32.u_free.dtype == torch.float32
    u32 = to_ref(m32, m32.u_free)
    print("fp32 model against the fp64 path", np.abs(u32 - base["us"][3]).max() / np.abs(u).max())
    assert np.abs(u32 - base["us"][3]).max() <= 1e-5 * np.abs(u).max()


def test_refusals_on_the_device():
    from hidenn_fem_amd.dynamics import NewmarkSolver
    from hidenn_fem_amd.mesh import structured_quad_mesh
    from hidenn_fem_amd.modal import ModalSolver
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.newton import NewtonKrylovSolver
    from hidenn_fem_amd.plasticity import ElastoplasticSolver
    from hidenn_fem_amd.radapt import RAdaptiveSolver
    from hidenn_fem_amd.solve import FrozenMeshSolver
    from hidenn_fem_amd.topopt import TopologyOptimizer
    from hidenn_fem_amd.loss import EnergyLoss2D
    m, s, _ = make("17x9")
    lf = s.loss_fn
    with pytest.raises(NotImplementedError, match="ElastoplasticSolver"):
        lf(m)
    for build in (lambda: FrozenMeshSolver(m, lf), lambda: NewmarkSolver(m, lf, 1e-3), lambda: ModalSolver(m, lf),
                  lambda: TopologyOptimizer(m, lf, 0.4), lambda: RAdaptiveSolver(m, lf), lambda: NewtonKrylovSolver(m, lf)):
        with pytest.raises(NotImplementedError):
            build()
    with pytest.raises(NotImplementedError):
        ElastoplasticSolver(m, EnergyLoss2D(device=dev(), dtype=F64))
    q = structured_quad_mesh(5, 4, dtype=F64)
    with pytest.raises(NotImplementedError):
        ElastoplasticSolver(PiecewiseLinearShapeNN2D(q[0], q[1]).to(dev()), lf)
    with pytest.raises(ValueError):
        ElastoplasticSolver(m, lf, precond="amg_tangent")


def test_the_example_runs(capsys):
    from examples.example4 import run_plasticity
    model, infos = run_plasticity(nx=40, ny=20, n_steps=2, precond="amg")
    out = capsys.readouterr().out
    print(out)
    assert len(infos) == 4 and all(i.converged for i in infos)
    assert out.count("plastic fraction") == 4 and "max alpha" in out
