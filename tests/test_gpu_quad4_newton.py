"""The QUAD4 Neo-Hookean tangent and the Newton-Krylov solve on it on the device (csrc/quad4_hyper_cg.hip, csrc/cg.hip,
hidenn_fem_amd.newton.Quad4NewtonKrylovSolver) against their CPU statement (tests/quad4_newton_reference.py, pinned on its own
by tests/test_quad4_newton_reference_host.py).

Meshes: those of tests/test_gpu_quad4_neo_hookean.py, the smallest that reach each kernel path -- ``tiny`` (one tile),
``grid33`` at tile_elems=64 (many tiles, halo cells) and at the default tile size, ``mixed`` (rotated corners, half the cells
clockwise, valence 1..9), the 17 x 9 ``plate`` (free and fixed rows mixed) at both tile sizes, ``jittered_x10`` at
tile_elems=4096 (a tile of 990 slots, more than the EPT x BLOCK = 768 the apply kernel prefetches: the plain loop behind the
prefetched records) -- and ``grid40``, 40 x 40 nodes at tile_elems=4096 (more than 768 local nodes: the fourth row-map register
in use, the largest LDS footprint a plan reaches).  Tolerances are tests/test_gpu_newton.py's: 1e-10 max|.| on q and the
diagonal blocks (the project's gradient tolerance: the same LDS-atomic accumulation), p^T q within 1e-10 sum|p_i q_i| (the form
is indefinite)."""
import ctypes as C

import pytest
import torch

import newton_reference as N
import quad4_hyper_reference as Q
import quad4_newton_reference as QN

F64, F32 = torch.float64, torch.float32
pytestmark = pytest.mark.gpu
CASES = [("tiny", 0), ("grid33", 64), ("grid33", 0), ("mixed", 0), ("plate", 0), ("plate", 64), ("jittered_x10", 4096),
         ("grid40", 4096)]
IDS = [f"{n}-{t}" for n, t in CASES]
_cache = {}


def dev():
    return torch.device("cuda:0")


def mesh(name):
    if "meshes" not in _cache:
        from hidenn_fem_amd.mesh import structured_quad_mesh
        ms = Q.meshes()
        j = ms["jittered"]
        ms["jittered_x10"] = (j[0], j[1].repeat(10, 1)) + tuple(j[2:])
        ms["tiny"] = structured_quad_mesh(5, 4, dtype=F64)
        ms["grid33"] = structured_quad_mesh(33, 17, jitter=Q.JITTER, seed=Q.SEED, dtype=F64)
        ms["grid40"] = structured_quad_mesh(40, 40, dtype=F64)
        _cache["meshes"] = ms
    return _cache["meshes"][name]


def make_model(name, u, dtype=F64, coords=None):
    """``plate``: boundary coordinates fixed, Dirichlet rows on the left with the values of ``u`` there, Neumann edges on the
    right; the others: every row free, no edges.  u_full = ``u`` [Nn, 2] by node id."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    c0, conn, geom, bc, _, edges = mesh(name)
    coords = c0 if coords is None else coords
    if name == "plate":
        m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=u[bc].to(dtype),
                                     neumann_edges=edges)
        free_u = u[~bc]
    else:
        m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn)
        free_u = u
    assert isinstance(m, QuadShapeNN2D)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(free_u.to(dtype), "u"))
    return m.to(dev())


def make_loss(dtype=F64, tile_elems=0, **kw):
    from hidenn_fem_amd.loss import Quad4NeoHookeanLoss2D
    return Quad4NeoHookeanLoss2D(device=dev(), dtype=dtype, tile_elems=tile_elems, **kw)


def make_solver(m, lf, **kw):
    from hidenn_fem_amd.newton import Quad4NewtonKrylovSolver
    return Quad4NewtonKrylovSolver(m, lf, **kw)


def free_mask(name):
    coords, _, _, bc = mesh(name)[:4]
    return ~bc if name == "plate" else torch.ones(coords.shape[0], dtype=torch.bool)


def reference_K(name, u, dtype=F64, E=10e9, key=None):
    """K_T over the free rows (node order) at u_full = ``u``, on the inputs as a model of ``dtype`` holds them; with ``key``
    computed once and never modified."""
    if key is not None and (name, key, dtype) in _cache:
        return _cache[(name, key, dtype)]
    coords, conn = mesh(name)[:2]
    lam, mu = Q.lame(E=E)
    K = N.restrict(QN.dense_tangent(coords.to(dtype).to(F64), u.to(dtype).to(F64), conn, lam, mu), free_mask(name))
    if key is not None:
        _cache[(name, key, dtype)] = K
    return K


def random_p(n, seed=5):
    return torch.rand(n, 2, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 0.5


def to_dev(m, rows):
    return m.from_caller_order(rows, "u").to(dev()).contiguous()


def to_ref(m, rows):
    return m.to_caller_order(rows.detach(), "u").cpu().double()


def check_apply(s, m, K, what):
    p = random_p(K.shape[0] // 2)
    q, pq = s.apply(to_dev(m, p))
    q = to_ref(m, q)
    want = (K @ p.reshape(-1)).reshape(-1, 2)
    eq = ((q - want).abs().max() / want.abs().max()).item()
    epq = abs(pq.item() - (p * want).sum().item()) / (p * want).abs().sum().item()
    print(what, "q", f"{eq:.2e}", "p^T q", f"{epq:.2e}")
    assert eq <= 1e-10 and epq <= 1e-10
    return p, want


# ---------------------------------------------------------------- 0. the shapes are the intended ones
def test_plan_shapes_cover_the_kernel_paths():
    """A tile of more slots than the apply kernel prefetches (3 x 256); tiles of more than 768 local nodes, whose LDS sums
    (the driver's: 48 B per local node + 16 B per owned row + 48 B for the apply, 32 + 24 + 64 for the blocks) stay within
    64 KiB."""
    z = lambda name: torch.zeros_like(mesh(name)[0])
    big = make_model("jittered_x10", z("jittered_x10")).tile_plan(4096).stats
    assert big["max_tile_elems"] > 3 * 256
    st = make_model("grid40", z("grid40")).tile_plan(4096).stats
    lds_apply = 48 * st["max_tile_nodes"] + 16 * st["max_tile_owned"] + (256 // 64 + 2) * 8
    lds_diag = 32 * st["max_tile_nodes"] + 24 * st["max_tile_owned"] + 2 * (256 // 64) * 8
    print("grid40 local nodes", st["max_tile_nodes"], "owned", st["max_tile_owned"], "LDS", lds_apply, lds_diag)
    assert st["max_tile_nodes"] > 768
    assert lds_apply <= 64 * 1024 and lds_diag <= 64 * 1024
    many = make_model("grid33", z("grid33")).tile_plan(64).stats
    assert many["n_tiles"] >= 8 and many["max_tile_nodes"] > many["max_tile_owned"]


# ---------------------------------------------------------------- 1. apply
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_apply_equals_the_dense_tangent(name, tile, dtype):
    """At the finite-strain field (K_T indefinite: tests/test_quad4_newton_reference_host.py) and at u = 0."""
    coords = mesh(name)[0]
    lf = make_loss(dtype=dtype, tile_elems=tile)
    for tag, u in (("field", Q.field(coords)), ("zero", torch.zeros_like(coords))):
        m = make_model(name, u, dtype)
        s = make_solver(m, lf)
        check_apply(s, m, reference_K(name, u, dtype, key=tag), f"{name}-{tile} {tag} {dtype}")
        assert s.info[1].item() == 0


# ---------------------------------------------------------------- 2. diagonal blocks
@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_diag_equals_the_diagonal_blocks(name, tile):
    coords = mesh(name)[0]
    u = Q.field(coords)
    m = make_model(name, u)
    s = make_solver(m, make_loss(tile_elems=tile))
    s.apply(to_dev(m, random_p(s.n_u)))
    want = N.diag_blocks(reference_K(name, u, key="field"))
    err = ((to_ref(m, s.diag) - want).abs().max() / want.abs().max()).item()
    print(name, tile, "diag", f"{err:.2e}")
    assert err <= 1e-10
    lam, mu = Q.lame()
    assert abs(s.info[0].item() - Q.element_terms(coords, u, mesh(name)[1], lam, mu)["J"].min().item()) <= 1e-13


def test_a_block_that_is_not_positive_definite_is_the_identity_in_the_preconditioner():
    """``Q.field`` gives no such block on these meshes; the field is scaled in steps of 0.25 until the CPU statement shows one
    (scale 2.0 on the plate; a few cells are inverted there and contribute zero blocks, also to the reference).  The
    preconditioner's effect is read off a CG start: at its breakdown-free iteration 0, z = M r is what one iteration moves
    along."""
    name = "plate"
    coords = mesh(name)[0]
    scale, bad = 1.0, None
    while scale <= 4.0:
        u = scale * Q.field(coords)
        blocks = N.diag_blocks(reference_K(name, u))
        dinv, pd = N.jacobi_inverse(blocks)
        if (~pd).any():
            bad = torch.nonzero(~pd)[:, 0]
            break
        scale += 0.25
    assert bad is not None
    print("scale", scale, "rows whose block is not positive definite", bad.tolist())
    m = make_model(name, u)
    s = make_solver(m, make_loss())
    g = random_p(s.n_u, seed=9)
    s.apply(to_dev(m, g))                                            # linearises at u
    err = ((to_ref(m, s.diag) - blocks).abs().max() / blocks.abs().max()).item()
    assert err <= 1e-10
    z = to_ref(m, s._precondition(to_dev(m, g)))
    want = N.apply_blocks(dinv, g)
    assert torch.equal(z[bad], g[bad])                               # identity rows
    assert ((z - want).abs().max() / want.abs().max()).item() <= 1e-9
    # and on the device's own path: one CG iteration from d = 0 moves along p = z = -M g
    s._g.copy_(to_dev(m, g))
    s._delta.zero_()
    from hidenn_fem_amd import _lib
    check = _lib.check
    stream = _lib.stream_ptr(dev())
    check(_lib.lib().hfem_cg_start(s._h, s._g.data_ptr(), s._g.data_ptr(), 1e-30, 0.0, 1, stream), "start")
    check(_lib.lib().hfem_cg_iterate(s._h, s._delta.data_ptr(), 1, stream), "iterate")
    st = s._read_status()
    d = to_ref(m, s._delta)
    if st[4] == 4.0:                                                 # p^T K p <= 0 on this direction: d did not move
        assert d.abs().max() == 0
    else:
        alpha = st[5]
        assert ((d + alpha * want).abs().max() / (alpha * want).abs().max()).item() <= 1e-9
        assert ((d[bad] + alpha * g[bad]).abs().max() / (alpha * g).abs().max()).item() <= 1e-12


# ---------------------------------------------------------------- 3. one inverted cell
@pytest.mark.parametrize("name,tile", [("jittered", 0), ("plate", 64)], ids=["jittered-0", "plate-64"])
def test_inverted_cell(name, tile):
    coords, conn = mesh(name)[:2]
    v, _ = Q.invert_one_cell(coords, Q.field(coords), conn)
    lam, mu = Q.lame()
    t = Q.element_terms(coords, v, conn, lam, mu)
    assert int(t["inverted"].sum()) == 1
    K = N.restrict(QN.dense_tangent(coords, v, conn, lam, mu, skip=t["inverted"]), free_mask(name))
    m = make_model(name, v)
    s = make_solver(m, make_loss(tile_elems=tile))
    check_apply(s, m, K, f"{name} inverted")
    assert s.info[1].item() == 1.0 and abs(s.info[0].item() - t["J"].min().item()) <= 1e-13
    assert torch.isfinite(s.diag).all()
    before = m.u_free.detach().clone()
    info = s.solve()
    assert info.reason == "inverted" and not info.converged and info.newton_iterations == 0
    assert torch.equal(m.u_free.detach(), before)


# ---------------------------------------------------------------- 4. iteration mode against the standalone apply
def test_one_graph_of_iterations_equals_pcg_composed_on_apply():
    """The plate at 0.05 x the field (K_T positive definite there, not at TRI3's 0.3: tests/test_quad4_newton_reference_host.py;
    asserted again on the host-composed recursion).  One captured graph of five iterations against five PCG iterations composed
    on the host from ``apply()`` and ``diag``: 1e-10."""
    from hidenn_fem_amd import _lib
    name = "plate"
    coords = mesh(name)[0]
    m = make_model(name, 0.05 * Q.field(coords))
    s = make_solver(m, make_loss(), iters_per_graph=5)
    g = to_dev(m, random_p(s.n_u, seed=13))
    s.apply(g)                                                       # refresh + linearise
    dinv, pd = N.jacobi_inverse(s.diag.cpu())
    assert pd.all()
    dinv = dinv.to(dev())
    d, r = torch.zeros_like(g), -g.clone()
    z = N.apply_blocks(dinv, r)
    rho, p = (r * z).sum(), torch.zeros_like(g)
    beta = 0.0
    for _ in range(5):
        p = z + beta * p
        q, pq = s.apply(p.contiguous())
        assert pq.item() > 0
        alpha = rho / pq
        d, r = d + alpha * p, r - alpha * q
        z = N.apply_blocks(dinv, r)
        rho_new = (r * z).sum()
        beta, rho = rho_new / rho, rho_new
    s._g.copy_(g)
    s._delta.zero_()
    _lib.check(_lib.lib().hfem_cg_start(s._h, s._g.data_ptr(), s._g.data_ptr(), 1e-30, 0.0, 1000,
                                        _lib.stream_ptr(dev())), "hfem_cg_start")
    torch.cuda.synchronize()
    s._replay()
    st = s._read_status()
    err = ((s._delta - d).abs().max() / d.abs().max()).item()
    print("iterations", st[0], "delta", f"{err:.2e}", "|r|", st[1], r.norm().item())
    assert st[0] == 5.0 and st[10] == 0.0
    assert err <= 1e-10 and abs(st[1] - r.norm().item()) <= 1e-10 * g.norm().item()


# ---------------------------------------------------------------- 5. the three Newton runs
def run_model(name, dtype=F64, coords=None):
    traction, loads, start, _ = N.RUNS[name]
    c0, _, _, bc = mesh("plate")[:4]
    u = torch.zeros_like(c0)
    if start == "field":
        u = Q.field(c0).clone()
        u[bc] = 0.0
    m = make_model("plate", u, dtype, coords)
    if not loads:
        t_force = lambda x: torch.zeros_like(x)
    elif traction is None:
        t_force = None
    else:
        t_force = lambda x: torch.stack([torch.full_like(x[:, 0], traction[0]), torch.full_like(x[:, 0], traction[1])], dim=1)
    return m, t_force


def run_kwargs(name):
    _, _, g_start = QN.reference_run(name)
    return dict(rtol=1e-10) if N.RUNS[name][1] else dict(rtol=0.0, atol=1e-10 * g_start)


RUN_CASES = [(n, p) for n in N.RUNS for p in ("block_jacobi", "amg")] + [("default", "none")]


@pytest.mark.parametrize("name,precond", RUN_CASES, ids=[f"{n}-{p}" for n, p in RUN_CASES])
def test_newton_runs(name, precond):
    """The runs of tests/test_quad4_newton_reference_host.py on the device, with tests/test_gpu_newton.py's assertions.  Stop:
    rtol = 1e-10 for the loaded runs; without loads ||g(u_free = 0)|| is identically 0, so the start's gradient norm (from the
    CPU statement) takes its place through atol = 1e-10 ||g(start)||, and in the 1e-8 bound below."""
    prob, ref, g_start = QN.reference_run(name)
    caps = N.RUNS[name][3]
    m, t_force = run_model(name)
    s = make_solver(m, make_loss(E=N.E_SOFT), t_force=t_force, precond=precond, **run_kwargs(name))
    info = s.solve()
    u_dev = to_ref(m, m.u_free)
    g_dev = prob.energy(u_dev)[1].norm().item()
    g_ref = prob.energy(ref.u)[1].norm().item()
    g0 = ref.rhs_norm if N.RUNS[name][1] else g_start
    lam_min = torch.linalg.eigvalsh(prob.tangent(ref.u))[0].item()
    du = (u_dev - ref.u).norm().item()
    print(name, precond, info.newton_iterations, info.cg_iterations, info.reason, "g_dev/g0", g_dev / g0, "du", du, "bound",
          2 * (g_dev + g_ref) / lam_min, [h["step"] for h in info.history], [h["cg_reason"] for h in info.history])
    assert info.converged and info.newton_iterations <= caps[0] and info.cg_iterations <= caps[1]
    assert abs(info.rhs_norm - ref.rhs_norm) <= 1e-10 * max(ref.rhs_norm, g_start)
    assert g_dev <= 1e-8 * g0
    assert lam_min > 0 and du <= 2 * (g_dev + g_ref) / lam_min
    e = [h["energy"] for h in info.history] + [info.energy]
    assert all(b <= a + 4 * N.EPS * abs(a) for a, b in zip(e, e[1:]))
    assert all(h["min_J"] > 0 for h in info.history)
    if name == "relax":
        assert any(h["cg_reason"] == "breakdown" for h in info.history)
    if name == "down":                                               # the line-search case
        assert info.history[0]["step"] < 1.0


# ---------------------------------------------------------------- 6. contract
def test_contract():
    name = "default"
    m, t_force = run_model(name)
    m.node_coords_free.grad = torch.full_like(m.node_coords_free, 3.0)
    m.u_free.grad = torch.full_like(m.u_free, 5.0)
    x0, xf0 = m.node_coords_free.detach().clone(), m.node_coords_fixed.detach().clone()
    ufix0 = m.u_fixed_rows().detach().clone()
    s = make_solver(m, make_loss(E=N.E_SOFT), t_force=t_force, rtol=1e-10)
    first = s.solve()
    assert first.converged and first.newton_iterations > 0
    assert torch.equal(m.node_coords_free.detach(), x0) and torch.equal(m.node_coords_fixed.detach(), xf0)
    assert torch.equal(m.u_fixed_rows().detach(), ufix0)
    assert (m.node_coords_free.grad == 3.0).all() and (m.u_free.grad == 5.0).all()
    again = s.solve()
    assert again.converged and again.newton_iterations == 0 and again.cg_iterations == 0
    key = s._key
    with torch.no_grad():
        m.u_fixed.add_(1e-3)
    moved = s.solve()
    assert s._key != key and moved.converged and moved.newton_iterations > 0
    assert torch.allclose(s._ufix, m.u_fixed_rows().detach().double())


def test_fp32_model_equals_the_fp64_solve_rounded_once():
    """An fp32 model against an fp64 model holding the same (fp32-rounded) coordinates, both under an fp32 loss (its rules'
    tables): every entry within one rounding (2^-24 |u|) plus 1e-9 max|u| for the two solves' stopping points."""
    name = "default"
    coords32 = mesh("plate")[0].to(F32).to(F64)
    lf = make_loss(dtype=F32, E=N.E_SOFT)
    m32, _ = run_model(name, F32)
    m64, _ = run_model(name, F64, coords32)
    a = make_solver(m32, lf, rtol=1e-10).solve()
    b = make_solver(m64, lf, rtol=1e-10).solve()
    assert m32.u_free.dtype == F32 and b.converged and a.newton_iterations > 0
    u32, u64 = m32.u_free.detach().double(), m64.u_free.detach()
    excess = ((u32 - u64).abs() - 2.0 ** -24 * u64.abs()).max().item() / u64.abs().max().item()
    print("fp32 excess over one rounding", excess, "grad", a.grad_norm / a.rhs_norm)
    assert excess <= 1e-9


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver, newton_solve_, quad4_newton_solve_
    coords = mesh("plate")[0]
    m = make_model("plate", torch.zeros_like(coords))
    lf = make_loss()
    t = structured_tri_mesh(5, 4, dtype=F64)
    tri = PiecewiseLinearShapeNN2D(t[0], t[1]).to(dev())
    for model, loss in ((tri, lf), (m, NeoHookeanLoss2D(device=dev(), dtype=F64)), (m, EnergyLoss2D(device=dev(), dtype=F64))):
        with pytest.raises(NotImplementedError):
            Quad4NewtonKrylovSolver(model, loss)
        with pytest.raises(NotImplementedError):
            quad4_newton_solve_(model, loss)
    free = make_model("tiny", torch.zeros_like(mesh("tiny")[0]))
    with pytest.raises(ValueError):
        Quad4NewtonKrylovSolver(free, lf, precond="amg")
    with pytest.raises(ValueError):
        Quad4NewtonKrylovSolver(m, lf, precond="ilu")
    for loss in (lf, NeoHookeanLoss2D(device=dev(), dtype=F64)):     # the TRI3 class keeps refusing QUAD4 models
        with pytest.raises(NotImplementedError, match="Quad4NewtonKrylovSolver"):
            NewtonKrylovSolver(m, loss)
        with pytest.raises(NotImplementedError):
            newton_solve_(m, loss)
    # the C entry points
    plan = m.tile_plan(0)
    n_u = int(m.u_free.shape[0])
    h = C.c_void_p()
    assert _lib.lib().hfem_cg_create_hyper(plan.handle, n_u - 1, C.byref(h)) == -1
    assert "n_u" in _lib.lib().hfem_last_error().decode() and not h.value
    # a solver of one kind refuses the other kind's setup
    s = make_solver(m, lf)
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    assert _lib.lib().hfem_cg_setup(s._h, s._xf.data_ptr(), s._xfix.data_ptr(), mat, 0.5, 1, None, None) == -1
    assert "hfem_cg_setup_hyper" in _lib.lib().hfem_last_error().decode()


def test_a_tile_beyond_64_kib_of_lds_never_gets_a_plan():
    """32 x 32 nodes in one tile would need 1024 local nodes, all owned: the planner refuses to build that device plan (as for
    the energy launch), so ``hfem_cg_create_hyper``'s own LDS check is a guard no device plan reaches."""
    from hidenn_fem_amd.mesh import structured_quad_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    q = structured_quad_mesh(32, 32, dtype=F64)
    with pytest.raises(RuntimeError, match="LDS"):
        make_solver(PiecewiseLinearShapeNN2D(q[0], q[1]).to(dev()), make_loss(tile_elems=4096))
