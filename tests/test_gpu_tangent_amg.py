"""The assembled Neo-Hookean tangent and the AMG hierarchy built on it (csrc/tri3_amg.hip
amg_assemble_hyper_kernel / hfem_amg_setup_hyper, hidenn_fem_amd.newton.assemble_tangent, precond="amg_tangent") against the
CPU statements of tests/tangent_amg_reference.py, tests/newton_reference.py and tests/quad4_newton_reference.py.

Tolerances: 1e-10 max|K| on the assembled matrix (what tests/test_gpu_newton.py gives the tangent apply), 1e-12 max|q| between
the assembled and the matrix-free product, 1e-12 against assemble_stiffness at u = 0; the end states of the Newton runs within
the existing tests' bound 2 (g_dev + g_ref) / lambda_min of the CPU run."""
import numpy as np
import pytest
import torch

import hyper_reference as H
import newton_reference as N
import quad4_hyper_reference as Q
import quad4_newton_reference as QN
import tangent_amg_reference as TA
from oracle import ref_chain as R

F64, F32 = torch.float64, torch.float32
pytestmark = pytest.mark.gpu
KINDS = ["tri", "quad"]
MESHES = [("tri", n) for n in ("jittered", "delaunay", "plate")] + [("quad", n) for n in ("jittered", "split", "mixed", "plate")]
MESH_IDS = [f"{k}-{n}" for k, n in MESHES]
HISTORY_KEYS = {"energy", "grad_norm", "eta", "cg_iterations", "cg_reason", "step", "min_J"}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cached_ramps():
    """The ramps (models and solvers with device handles) are shared by the tests of this module and freed with it."""
    yield
    for key in [k for k in _cache if isinstance(k, tuple)]:
        del _cache[key]


def dev():
    return torch.device("cuda:0")


def mesh(kind, name):
    if kind not in _cache:
        from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
        ms = H.meshes() if kind == "tri" else Q.meshes()
        ms["plate121"] = (structured_tri_mesh if kind == "tri" else structured_quad_mesh)(121, 61, dtype=F64)
        _cache[kind] = ms
    return _cache[kind][name]


def make_model(kind, name, u, dtype=F64):
    """Boundary coordinates fixed, Dirichlet rows as the mesh marks them with the values of ``u`` there (nonzero for the
    test field), the mesh's Neumann edges.  u_full = ``u`` [Nn, 2] by node id."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    coords, conn, geom, bc, _, edges = mesh(kind, name)
    assert bc.any() and not bc.all()
    m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=u[bc].to(dtype),
                                 neumann_edges=edges)
    assert getattr(m, "nodes_per_element", 3) == (3 if kind == "tri" else 4)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(u[~bc].to(dtype), "u"))
    return m.to(dev())


def make_loss(kind, dtype=F64, **kw):
    from hidenn_fem_amd.loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    return (NeoHookeanLoss2D if kind == "tri" else Quad4NeoHookeanLoss2D)(device=dev(), dtype=dtype, **kw)


def make_solver(kind, m, lf, **kw):
    from hidenn_fem_amd.newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver
    return (NewtonKrylovSolver if kind == "tri" else Quad4NewtonKrylovSolver)(m, lf, **kw)


def reference_K(kind, name, u, m, dtype=F64, E=10e9, skip=None):
    """The sparse CPU statement over the model's free rows in storage order, on the inputs as a model of ``dtype`` holds them."""
    coords, conn = mesh(kind, name)[:2]
    lam, mu = H.lame(E=E)
    W = float(R.triangle_gauss(4, dtype)[1].to(F64).sum()) if kind == "tri" else None
    return TA.sparse_tangent(coords.to(dtype).to(F64), u.to(dtype).to(F64), conn, lam, mu, W, np.asarray(m._u_src), skip)


def dense(K):
    return K.to_dense().cpu().numpy()


def const_traction(tx, ty):
    return lambda x: torch.stack([torch.full_like(x[:, 0], tx), torch.full_like(x[:, 0], ty)], dim=1)


def to_ref(m, rows):
    return m.to_caller_order(rows.detach(), "u").cpu().double()


# ---------------------------------------------------------------- 1. assemble_tangent against the sparse reference
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,name", MESHES, ids=MESH_IDS)
def test_assembled_tangent_equals_the_sparse_reference(kind, name, dtype):
    from hidenn_fem_amd.newton import assemble_tangent
    u = H.field(mesh(kind, name)[0])
    m = make_model(kind, name, u, dtype)
    lf = make_loss(kind, dtype)
    K = assemble_tangent(m, lf)
    assert K.layout == torch.sparse_bsr and K.dtype == F64 and K.values().shape[1:] == (2, 2)
    want = reference_K(kind, name, u, m, dtype).toarray()
    got = dense(K)
    assert got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print(kind, name, dtype, "assembled K_T against the sparse reference", f"{err:.2e}")
    assert err <= 1e-10
    again = assemble_tangent(m, lf)
    assert torch.equal(K.values(), again.values()) and torch.equal(K.col_indices(), again.col_indices())
    assert torch.equal(K.crow_indices(), again.crow_indices())


@pytest.mark.parametrize("kind", KINDS)
def test_an_inverted_element_contributes_zeros(kind):
    from hidenn_fem_amd.newton import assemble_tangent
    name = "jittered"
    coords, conn = mesh(kind, name)[:2]
    lam, mu = H.lame()
    if kind == "tri":
        v, _ = H.invert_one_element(coords, H.field(coords), conn)
        inverted = H.element_terms(coords, v, conn, lam, mu, H.tri_W())["inverted"]
    else:
        v, _ = Q.invert_one_cell(coords, H.field(coords), conn)
        inverted = Q.element_terms(coords, v, conn, lam, mu)["inverted"]
    assert int(inverted.sum()) == 1
    m = make_model(kind, name, v)
    got = dense(assemble_tangent(m, make_loss(kind)))
    want = reference_K(kind, name, v, m, skip=inverted).toarray()         # the rest unchanged
    assert np.abs(reference_K(kind, name, v, m).toarray() - want).max() == 0.0   # the statement's own rule gives the same
    err = np.abs(got - want).max() / np.abs(want).max()
    print(kind, "one inverted element", f"{err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("kind,name", MESHES, ids=MESH_IDS)
def test_at_zero_displacement_the_tangent_is_the_linear_stiffness(kind, name):
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.newton import assemble_tangent
    from hidenn_fem_amd.solve import assemble_stiffness
    m = make_model(kind, name, torch.zeros_like(mesh(kind, name)[0]))
    KT = assemble_tangent(m, make_loss(kind))
    KL = assemble_stiffness(m, EnergyLoss2D(device=dev(), dtype=F64, grad_convention="physical"))
    assert torch.equal(KT.crow_indices(), KL.crow_indices()) and torch.equal(KT.col_indices(), KL.col_indices())
    err = ((KT.values() - KL.values()).abs().max() / KL.values().abs().max()).item()
    print(kind, name, "K_T(0) against assemble_stiffness", f"{err:.2e}")
    assert err <= 1e-12


# ---------------------------------------------------------------- 2. assembled against matrix-free
def _delaunay_tile_major():
    from hidenn_fem_amd.mesh import unstructured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nc, conn, geom, bc, mn, edges = unstructured_tri_mesh(6000, dtype=F64)
    u = H.field(nc)
    m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=u[bc], neumann_edges=edges)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(u[~bc], "u"))
    return m.to(dev())


def _quad_off_default_tile():
    from test_gpu_quad4_shapes import _mesh, _new_model
    m = _new_model("S", dev())
    nc, bc = _mesh("S")[0][0], _mesh("S")[0][3]
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(H.field(nc)[~bc], "u").to(dev()))
    return m


@pytest.mark.parametrize("kind", KINDS)
def test_assembled_product_equals_the_matrix_free_apply(kind):
    """TRI3: a Delaunay model with tile-major rows over more than one tile; QUAD4: the 61 x 45 jittered grid at tile_elems=800
    (more than 768 local nodes and cells in a tile: the <4, 4> apply instance, off the default tile shape)."""
    from hidenn_fem_amd.newton import assemble_tangent
    if kind == "tri":
        m, lf = _delaunay_tile_major(), make_loss("tri")
        assert m.row_order == "tile"
    else:
        m, lf = _quad_off_default_tile(), make_loss("quad", tile_elems=800)
    s = make_solver(kind, m, lf)
    assert s.plan.n_tiles > 1
    if kind == "quad":
        st = s.plan.stats
        assert st["max_tile_nodes"] > 768 and st["max_tile_elems"] > 768
    K = assemble_tangent(m, lf)
    p = torch.randn(m.u_free.shape, dtype=F64, device=dev(), generator=torch.Generator(device=dev()).manual_seed(3))
    q, _ = s.apply(p)
    kp = (K @ p.reshape(-1, 1)).reshape(-1, 2)
    err = ((kp - q).abs().max() / q.abs().max()).item()
    print(kind, "K_T p against apply", f"{err:.2e}", "inverted", s.info[1].item())
    assert err <= 1e-12


# ---------------------------------------------------------------- 3. the near-null space of the tangent setup
@pytest.mark.parametrize("kind", KINDS)
def test_fine_near_null_space_is_at_the_deformed_position_and_returns(kind):
    coords, _, _, bc = mesh(kind, "plate")[:4]
    u = H.field(coords)
    m = make_model(kind, "plate", u)
    s = make_solver(kind, m, make_loss(kind), precond="amg_tangent")
    s._fresh()
    s._u.copy_(m.u_free.detach())
    a = s._amg
    a.setup_hyper(s._xf, s._xfix, s._u, s._ufix, s._lame, float(s.loss_fn._W))

    def expect(pos):
        p = m.from_caller_order(pos[~bc], "u")
        one, zero = torch.ones_like(p[:, 0]), torch.zeros_like(p[:, 0])
        return torch.stack([torch.stack([one, zero, -p[:, 1]], 1), torch.stack([zero, one, p[:, 0]], 1)], 1).reshape(-1)

    for tag, pos in (("deformed", coords + u), ("undeformed", coords)):
        got, want = a.values(0, 3).cpu(), expect(pos)
        err = ((got - want).abs().max() / want.abs().max()).item()
        print(kind, tag, "near-null space", err)
        assert err <= 1e-15
        s._small_strain_setup()                                        # hfem_amg_setup on the same handle


# ---------------------------------------------------------------- 5. the iteration count (and 4. the cycle at that state)
def ramp(kind):
    """The 121 x 61 plate, E = 2e6, left edge clamped, traction (0, -4e4) in 10 equal increments from u = 0 with
    precond="amg_tangent", rtol 1e-8; computed once.  -> dict(model, loss, solver, infos, kinds at the converged states)"""
    if ("ramp", kind) not in _cache:
        coords = mesh(kind, "plate121")[0]
        m = make_model(kind, "plate121", torch.zeros_like(coords))
        lf = make_loss(kind, E=N.E_SOFT)
        s = make_solver(kind, m, lf, precond="amg_tangent", rtol=1e-8)
        infos, kinds, before = [], [], []
        for k in range(1, 11):
            s.t_force = const_traction(0.0, -4e4 * k / 10)
            s.refresh()
            infos.append(s.solve())
            before.append(dict(s.amg))
            s._tangent_setup()                                         # a setup AT the converged state
            kinds.append(s._amg_kind)
        _cache[("ramp", kind)] = dict(model=m, loss=lf, solver=s, infos=infos, kinds=kinds, reports=before,
                                      t_force=const_traction(0.0, -4e4))
    return _cache[("ramp", kind)]


@pytest.mark.parametrize("kind", KINDS)
def test_tangent_hierarchy_halves_the_iterations_of_the_small_strain_one(kind):
    """At the ramp's final state, K_T d = b for one seeded b to rtol 1e-8 by the three preconditioners on the same model.
    TRI3: 2 its(amg_tangent) <= its(amg) -- the two-level CPU restatement gives 4.9 (84 / 17, 79 / 16), which leaves 2.4 x
    for the multi-level cycle and the library's own aggregation.  QUAD4 (no CPU number): its(amg_tangent) < its(amg)."""
    r = ramp(kind)
    m, lf = r["model"], r["loss"]
    for k, (info, at_end) in enumerate(zip(r["infos"], r["kinds"])):
        print(kind, "increment", k + 1, info.newton_iterations, info.cg_iterations, info.reason, "min J", info.min_J,
              [h["amg"] for h in info.history], "at the converged state:", at_end)
    assert all(i.converged for i in r["infos"])
    assert all(k == "tangent" for k in r["kinds"])                     # no fallback at the converged states
    assert r["solver"].amg["levels"] >= 3
    b = torch.randn(m.u_free.shape, dtype=F64, device=dev(), generator=torch.Generator(device=dev()).manual_seed(11))
    out = {}
    for precond in ("amg_tangent", "amg", "block_jacobi"):
        s = make_solver(kind, m, lf, t_force=r["t_force"], precond=precond)
        d, its, reason = s.linear_solve(b, 1e-8)
        assert reason == "rtol", (precond, reason)
        if precond == "amg_tangent":
            assert s._amg_kind == "tangent" and s.amg["fallbacks_coarse"] == 0
        out[precond] = (d, its)
    its = {p: v[1] for p, v in out.items()}
    top = out["amg_tangent"][0].abs().max().item()
    dev_a = (out["amg"][0] - out["amg_tangent"][0]).abs().max().item() / top
    dev_j = (out["block_jacobi"][0] - out["amg_tangent"][0]).abs().max().item() / top
    print(kind, "linear_solve iterations", its, "ratio", its["amg"] / its["amg_tangent"], "deviation of d", dev_a, dev_j)
    if kind == "tri":
        assert 2 * its["amg_tangent"] <= its["amg"]
    else:
        assert its["amg_tangent"] < its["amg"]
    assert dev_a <= 1e-6 and dev_j <= 1e-6


def test_vcycle_of_the_tangent_setup_is_symmetric_positive_and_bit_reproducible():
    """tests/test_gpu_amg.py's V-cycle checks after a tangent setup at the ramp's final state (three or more levels)."""
    r = ramp("tri")
    m, lf = r["model"], r["loss"]
    b = torch.zeros(m.u_free.shape, dtype=F64, device=dev())
    b[0, 0] = 1.0
    solvers = [make_solver("tri", m, lf, t_force=r["t_force"], precond="amg_tangent") for _ in range(2)]
    for s in solvers:
        s.linear_solve(b, 0.5, max_iter=1)                             # linearise + tangent setup
        assert s._amg_kind == "tangent" and s.amg["levels"] >= 3 and s.amg["tangent_setups"] == 1
    s, s2 = solvers
    g = torch.Generator(device=dev()).manual_seed(5)
    for _ in range(3):
        x = torch.randn(m.u_free.shape, dtype=F64, device=dev(), generator=g)
        y = torch.randn(m.u_free.shape, dtype=F64, device=dev(), generator=g)
        Mx, My = s._precondition(x), s._precondition(y)
        lhs, rhs = (x * My).sum().item(), (y * Mx).sum().item()
        assert abs(lhs - rhs) <= 1e-10 * x.norm().item() * My.norm().item()
        assert (x * Mx).sum().item() > 0.0
    z1, z2, z3 = s._precondition(x), s._precondition(x), s2._precondition(x)
    assert torch.equal(z1, z2) and torch.equal(z1, z3)
    assert torch.equal(s._amg.coarse_inv, s2._amg.coarse_inv)


# ---------------------------------------------------------------- 6. the reference runs on one level
def run_setup(kind, name):
    """Model, t_force, stopping keywords and the CPU run of ``N.RUNS[name]`` on the 17 x 9 plate."""
    traction, loads, start, caps = N.RUNS[name]
    prob, ref, g_start = (N if kind == "tri" else QN).reference_run(name)
    coords, _, _, bc = mesh(kind, "plate")[:4]
    u = torch.zeros_like(coords)
    if start == "field":
        u = H.field(coords).clone()
        u[bc] = 0.0
    m = make_model(kind, "plate", u)
    t_force = (lambda x: torch.zeros_like(x)) if not loads else None if traction is None else const_traction(*traction)
    kw = dict(rtol=1e-10) if loads else dict(rtol=0.0, atol=1e-10 * g_start)
    return m, t_force, kw, prob, ref, g_start


def check_end_state(name, m, info, prob, ref, g_start):
    u_dev = to_ref(m, m.u_free)
    g_dev, g_ref = prob.energy(u_dev)[1].norm().item(), prob.energy(ref.u)[1].norm().item()
    g0 = ref.rhs_norm if N.RUNS[name][1] else g_start
    lam_min = torch.linalg.eigvalsh(prob.tangent(ref.u))[0].item()
    du = (u_dev - ref.u).norm().item()
    print(name, info.newton_iterations, info.cg_iterations, info.reason, "g_dev/g0", g_dev / g0, "du", du, "bound",
          2 * (g_dev + g_ref) / lam_min, [h["step"] for h in info.history], [h["cg_reason"] for h in info.history],
          [h.get("amg") for h in info.history])
    assert info.converged and g_dev <= 1e-8 * g0
    assert lam_min > 0 and du <= 2 * (g_dev + g_ref) / lam_min
    e = [h["energy"] for h in info.history] + [info.energy]
    assert all(b <= a + 4 * N.EPS * abs(a) for a, b in zip(e, e[1:]))


@pytest.mark.parametrize("name", list(N.RUNS))
@pytest.mark.parametrize("kind", KINDS)
def test_reference_runs_on_a_one_level_hierarchy(kind, name):
    """The 17 x 9 plate is a one-level hierarchy: the coarse matrix is K_T itself, so safeguard (a) is an exact test of
    definiteness.  ``relax`` starts from an indefinite tangent: its first entries ran on the small-strain numbers."""
    m, t_force, kw, prob, ref, g_start = run_setup(kind, name)
    s = make_solver(kind, m, make_loss(kind, E=N.E_SOFT), t_force=t_force, precond="amg_tangent", **kw)
    info = s.solve()
    rep = s.amg
    assert rep["levels"] == 1
    check_end_state(name, m, info, prob, ref, g_start)
    assert all(set(h) == HISTORY_KEYS | {"amg"} and h["amg"] in ("tangent", "small_strain") for h in info.history)
    assert rep["tangent_setups"] == info.newton_iterations
    print(kind, name, {k: rep[k] for k in ("tangent_setups", "fallbacks_coarse", "fallbacks_descent")})
    if name == "relax":
        assert info.history[0]["amg"] == "small_strain" and rep["fallbacks_coarse"] >= 1
    else:
        assert info.history[-1]["amg"] == "tangent"


# ---------------------------------------------------------------- 7. robustness on three levels
def test_relaxation_from_the_field_on_three_levels():
    coords, conn, _, bc, _, edges = mesh("tri", "plate121")
    u = H.field(coords).clone()
    u[bc] = 0.0
    lam, mu = H.lame(E=N.E_SOFT)
    g_start = H.total(coords, u, conn, lam, mu, H.tri_W())["gU"][~bc].norm().item()
    m = make_model("tri", "plate121", u)
    s = make_solver("tri", m, make_loss("tri", E=N.E_SOFT), t_force=lambda x: torch.zeros_like(x), precond="amg_tangent",
                    rtol=0.0, atol=1e-10 * g_start)
    info = s.solve()
    rep = s.amg
    print("relax 121x61", info.newton_iterations, info.cg_iterations, info.reason, [h["amg"] for h in info.history],
          {k: rep[k] for k in ("tangent_setups", "fallbacks_coarse", "fallbacks_descent")})
    assert rep["levels"] >= 3 and info.converged
    assert all("amg" in h for h in info.history)
    e = [h["energy"] for h in info.history] + [info.energy]
    assert all(b <= a + 4 * N.EPS * abs(a) for a, b in zip(e, e[1:]))


# ---------------------------------------------------------------- 8. amg_rebuild="solve"
@pytest.mark.parametrize("kind", KINDS)
def test_rebuild_once_per_solve(kind):
    m, t_force, kw, prob, ref, g_start = run_setup(kind, "default")
    s = make_solver(kind, m, make_loss(kind, E=N.E_SOFT), t_force=t_force, precond="amg_tangent", amg_rebuild="solve", **kw)
    info = s.solve()
    assert info.newton_iterations > 1 and s.amg["tangent_setups"] == 1
    check_end_state("default", m, info, prob, ref, g_start)
    s.t_force = const_traction(1.5e5, 0.0)
    s.refresh()
    more = s.solve()
    assert more.converged and more.newton_iterations > 1 and s.amg["tangent_setups"] == 2
    assert all("amg" in h for h in info.history + more.history)


# ---------------------------------------------------------------- 9. contract and refusals
def test_contract_and_refusals():
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.newton import assemble_tangent
    for kind in KINDS:
        coords, conn = mesh(kind, "jittered")[:2]
        free = PiecewiseLinearShapeNN2D(coords, conn).to(dev())
        lf = make_loss(kind)
        with pytest.raises(ValueError, match="Dirichlet"):
            make_solver(kind, free, lf, precond="amg_tangent")
        m = make_model(kind, "plate", torch.zeros_like(mesh(kind, "plate")[0]))
        with pytest.raises(ValueError, match="amg_rebuild"):
            make_solver(kind, m, lf, precond="amg_tangent", amg_rebuild="never")
        with pytest.raises(NotImplementedError, match="assemble_stiffness"):
            assemble_tangent(m, EnergyLoss2D(device=dev(), dtype=F64))
        with pytest.raises(NotImplementedError, match="assemble_stiffness"):
            assemble_tangent(m, make_loss("quad" if kind == "tri" else "tri"))


@pytest.mark.parametrize("quad", [False, True], ids=KINDS)
def test_example4_ramp_runs_with_the_tangent_hierarchy(quad, capsys):
    """``python -m examples.example4 --neo-hookean --newton --precond amg_tangent [--quad]`` on 40 x 20 nodes, two load steps:
    every increment converges and its line shows the setup and fallback counts."""
    import examples.example4 as e4
    model, energy = e4.run_neo_hookean(nx=40, ny=20, load_steps=2, newton=True, precond="amg_tangent", quad=quad)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "tangent setups" in ln]
    print(out)
    assert len(lines) == 2 and all("fallbacks coarse" in ln and "descent" in ln for ln in lines)
    assert "halved" not in out and energy == energy and "load 1.0000" in lines[-1]


# (Newton, CG) iterations of the 17 x 9 ``default`` run with precond="amg" as the commit before this change printed them on an
# MI355X (tests/test_gpu_newton.py::test_newton_runs[default-amg] and tests/test_gpu_quad4_newton.py's twin, the same inputs)
AMG_COUNTS_BEFORE = {"tri": (6, 33), "quad": (5, 21)}


@pytest.mark.parametrize("kind", KINDS)
def test_small_strain_amg_is_unchanged(kind):
    m, t_force, kw, prob, ref, g_start = run_setup(kind, "default")
    s = make_solver(kind, m, make_loss(kind, E=N.E_SOFT), t_force=t_force, precond="amg", **kw)
    info = s.solve()
    print(kind, "amg default", info.newton_iterations, info.cg_iterations)
    assert all(set(h) == HISTORY_KEYS for h in info.history)
    assert set(s.amg) == {"levels", "rows", "block_rows", "block_nnz", "block_size", "operator_complexity",
                          "host_setup_seconds", "numeric_setup_seconds", "numeric_setups"}
    assert s.amg["numeric_setups"] == 1
    assert (info.newton_iterations, info.cg_iterations) == AMG_COUNTS_BEFORE[kind]
