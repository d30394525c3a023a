"""The QUAD4 Neo-Hookean total potential on the device (csrc/quad4_hyper.hip, hidenn_fem_amd.loss.Quad4NeoHookeanLoss2D)
against its CPU statement (tests/quad4_hyper_reference.py, pinned on its own by tests/test_quad4_hyper_reference_host.py).

Meshes on [0, 2] x [0, 1], the smallest shapes that exercise each path of the kernel:
(a) ``tiny``: 5 x 4 nodes, one tile;
(b) ``grid33``: 33 x 17 jittered nodes at tile_elems=64 (many tiles, halo cells) and at the default tile size;
(c) ``mixed``: the Delaunay mesh of 150 points split into quads, renumbered with rotated corners and half the cells clockwise
    (valence 1..9);
(d) ``plate``: the structured 17 x 9 plate with its masks (free and fixed rows mixed) and Neumann edges, at the default tile
    size and at tile_elems=64;
(e) ``jittered_x10``: the jittered 17 x 9 mesh with every cell listed ten times at tile_elems=4096 -- a tile of 990 slots,
    more than the EPT x BLOCK = 768 the kernel prefetches: the plain loop behind the prefetched records.
Field: u = (0.25 sin 2.1x cos 1.3y, 0.15 cos(1.7x + 0.3) sin 2.4y), min J >= 0.31 over all Gauss points.

Tolerances are the project's parity tolerances for this energy (tests/test_gpu_neo_hookean.py; kernel and statement differ in
summation order and fma contraction only): loss 1e-12 relative, gradients 1e-10 max|g|, min J 1e-13, fp32 rows within one
rounding of the fp64 result on the same float inputs."""
import ctypes as C
import math

import pytest
import torch

import quad4_hyper_reference as Q
from oracle import ref_chain as R

F64, F32 = torch.float64, torch.float32
pytestmark = pytest.mark.gpu
CASES = [("tiny", 0), ("grid33", 64), ("grid33", 0), ("mixed", 0), ("plate", 0), ("plate", 64), ("jittered_x10", 4096)]
IDS = [f"{n}-{t}" for n, t in CASES]
_cache = {}


def b_force(x):
    return torch.stack([2e9 * (1.0 + x[:, 0]), -1e9 * x[:, 1]], dim=1)


def t_force(x):
    return torch.stack([1e9 * (1.0 + x[:, 1]), 2e8 * x[:, 0]], dim=1)


def mesh(name):
    if "meshes" not in _cache:
        from hidenn_fem_amd.mesh import structured_quad_mesh
        ms = Q.meshes()
        j = ms["jittered"]
        ms["jittered_x10"] = (j[0], j[1].repeat(10, 1)) + tuple(j[2:])
        ms["tiny"] = structured_quad_mesh(5, 4, dtype=F64)
        ms["grid33"] = structured_quad_mesh(33, 17, jitter=Q.JITTER, seed=Q.SEED, dtype=F64)
        _cache["meshes"] = ms
    return _cache["meshes"][name]


def make_model(name, u=None, dtype=F64, free_coords=False):
    """``plate``: boundary coordinates fixed, Dirichlet rows on the left (their values are the field's), Neumann edges on the
    right; with ``free_coords`` every coordinate row is free.  The others: every row free, no edges.  u_full = ``u`` (default:
    the finite-strain field) at the nodes."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    coords, conn, geom, bc, _, edges = mesh(name)
    u = Q.field(coords) if u is None else u
    if name == "plate":
        m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn, boundary_mask=None if free_coords else geom, dirichlet_mask=bc,
                                     u_fixed=u[bc].to(dtype), neumann_edges=edges)
        free_u = u[~bc]
    else:
        m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn)
        free_u = u
    assert isinstance(m, QuadShapeNN2D)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(free_u.to(dtype), "u"))
    return m.to(torch.device("cuda:0"))


def make_loss(dtype=F64, tile_elems=0, **kw):
    from hidenn_fem_amd.loss import Quad4NeoHookeanLoss2D
    return Quad4NeoHookeanLoss2D(device=torch.device("cuda:0"), dtype=dtype, tile_elems=tile_elems, **kw)


def masks(name, free_coords=False):
    """(free-coordinate mask, free-displacement mask) by node id: the rows the model's parameters hold, in caller order."""
    coords, _, geom, bc = mesh(name)[:4]
    if name != "plate":
        z = torch.zeros(coords.shape[0], dtype=torch.bool)
        return ~z, ~z
    return (~geom if not free_coords else torch.ones_like(geom)), ~bc


def reference(name, forces="none", u=None, key=None, dtype=F64):
    """The CPU statement of one (mesh, forces[, field]) on the model's inputs; computed once per key, never modified.
    ``dtype=F32``: evaluated on the fp32-rounded parameters with the fp32 rule's traction table, as an fp32 model and loss hold
    them."""
    ck = (name, forces, key, dtype)
    if ck in _cache:
        return _cache[ck]
    coords, conn, _, _, _, edges = mesh(name)
    lam, mu = Q.lame()
    u = Q.field(coords) if u is None else u
    coords, u = coords.to(dtype).to(F64), u.to(dtype).to(F64)
    Bq = Q.body_points(b_force) if forces in ("body", "all") else None
    T = None
    if name == "plate":
        if dtype == F32:                                            # default traction only: the constant table of the fp32 rule
            xg1, wg1 = (t.to(F64) for t in R.interval_gauss(2, F32))
            ci, cj = float((wg1 * (1 - xg1)).sum()), float((wg1 * xg1).sum())
            T = torch.tensor([ci * 100e3, 0.0, cj * 100e3, 0.0], dtype=F64)
        else:
            T = Q.traction_table(coords, edges, t_force if forces in ("traction", "all") else None)
    r = Q.total(coords, u, conn, lam, mu, Bq, edges if name == "plate" else None, T)
    _cache[ck] = r
    return r


def run_autograd(m, lf, forces="none"):
    for p in (m.node_coords_free, m.u_free):
        p.grad = None
    loss = lf(m, b_force if forces in ("body", "all") else None, t_force if forces in ("traction", "all") else None)
    loss.backward()
    return loss.detach(), m.node_coords_free.grad, m.u_free.grad


def check(m, name, ref, loss, gx, gu, info, free_coords=False, what=""):
    mx, mu_ = masks(name, free_coords)
    gx = m.to_caller_order(gx.detach(), "x").cpu().double()
    gu = m.to_caller_order(gu.detach(), "u").cpu().double()
    rx, ru = ref["gX"][mx], ref["gU"][mu_]
    figs = dict(loss=abs(loss.item() - ref["loss"]) / abs(ref["loss"]) if math.isfinite(ref["loss"]) else float(loss.item() != ref["loss"]),
                gx=((gx - rx).abs().max() / ref["gX"].abs().max()).item(), gu=((gu - ru).abs().max() / ref["gU"].abs().max()).item(),
                minJ=abs(info[0].item() - ref["min_J"]), count=info[1].item())
    print(name, what, {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["loss"] <= 1e-12
    assert figs["gx"] <= 1e-10 and figs["gu"] <= 1e-10
    assert figs["minJ"] <= 1e-13 and figs["count"] == ref["count"]
    return figs


# ---------------------------------------------------------------- 0. the shapes are the intended ones
def test_plan_shapes_cover_the_kernel_paths():
    """One tile; many tiles with halo cells; a tile with more slots than the kernel prefetches (EPT x BLOCK = 3 x 256)."""
    assert make_model("tiny").tile_plan(0).n_tiles == 1
    st = make_model("grid33").tile_plan(64).stats
    assert st["n_tiles"] >= 8 and st["max_tile_nodes"] > st["max_tile_owned"]
    assert make_model("plate").tile_plan(64).n_tiles >= 2
    big = make_model("jittered_x10").tile_plan(4096).stats
    assert big["max_tile_elems"] > 3 * 256


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_parity_through_autograd(name, tile):
    m, lf = make_model(name), make_loss(tile_elems=tile)
    forces = ["none", "body"] + (["traction", "all"] if name == "plate" else [])
    for f in forces:
        loss, gx, gu = run_autograd(m, lf, f)
        assert loss.dtype == F64 and gx.dtype == F64
        check(m, name, reference(name, f), loss, gx, gu, lf.info, what=f"autograd/{f}")
    coords, conn = mesh(name)[:2]                                    # domain_energy: the edges off
    want = Q.total(coords, Q.field(coords), conn, *Q.lame(), Q.body_points(b_force))["loss"]
    assert abs(lf.domain_energy(m, b_force).item() - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_parity_through_value_and_grad(name, tile):
    m, lf = make_model(name), make_loss(tile_elems=tile)
    loss = lf.value_and_grad_(m)
    check(m, name, reference(name), loss, m.node_coords_free.grad, m.u_free.grad, lf.info, what="value_and_grad_")
    loss2, gx, gu = run_autograd(make_model(name), lf)
    assert torch.equal(loss2, loss)                                  # the same launch either way


def test_traction_that_moves_with_free_nodes_goes_through_autograd():
    """Every coordinate row of the plate free and a traction callable: the edge term is ``edge_energy`` through autograd
    (the traction is evaluated at points that move), the domain term the fused launch."""
    name = "plate"
    m, lf = make_model(name, free_coords=True), make_loss()
    loss, gx, gu = run_autograd(m, lf, "traction")
    coords, conn, _, _, _, edges = mesh(name)
    lam, mu = Q.lame()
    ref = dict(Q.total(coords, Q.field(coords), conn, lam, mu))
    x, u = coords.clone().requires_grad_(True), Q.field(coords).requires_grad_(True)
    xg1, wg1 = R.interval_gauss(2, F64)
    edge = -R.edge_energy(x, u, edges, xg1, wg1, t_force)
    edge.backward()
    ref.update(loss=ref["loss"] + edge.item(), gX=ref["gX"] + x.grad, gU=ref["gU"] + u.grad)
    check(m, name, ref, loss, gx, gu, lf.info, free_coords=True, what="moving traction")


# ---------------------------------------------------------------- 2. fp32 models
@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_fp32_models_round_once_on_store(name, tile):
    """Float rows widened on load, fp64 arithmetic, one rounding on store: every gradient entry within 2^-24 |g_i| + 1e-10
    max|g| of the fp64 statement on the fp32-rounded parameters; the loss (fp64, before any cast) within 1e-12 relative."""
    m, lf = make_model(name, dtype=F32), make_loss(dtype=F32, tile_elems=tile)
    ref = reference(name, dtype=F32)
    loss = lf.value_and_grad_(m)
    assert loss.dtype == F64 and m.u_free.grad.dtype == F32
    mx, mu_ = masks(name)
    print(name, "fp32 loss", abs(loss.item() - ref["loss"]) / abs(ref["loss"]))
    assert abs(loss.item() - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    for got, want, full, which in ((m.node_coords_free.grad, ref["gX"][mx], ref["gX"], "x"), (m.u_free.grad, ref["gU"][mu_], ref["gU"], "u")):
        got = m.to_caller_order(got, which).cpu().double()
        excess = ((got - want).abs() - 2.0 ** -24 * want.abs()).max().item() / full.abs().max().item()
        print(name, which, "excess over one rounding", f"{excess:.2e}")
        assert excess <= 1e-10
    assert abs(lf.info[0].item() - ref["min_J"]) <= 1e-13 and lf.info[1].item() == 0
    la, gx, gu = run_autograd(m, lf)
    assert la.dtype == F32 and gx.dtype == F32 and torch.equal(la, loss.to(F32))


# ---------------------------------------------------------------- 3. patch and objectivity
@pytest.mark.parametrize("name,tile", [("grid33", 64), ("mixed", 0)], ids=["grid33-64", "mixed-0"])
def test_patch_and_objectivity_on_the_device(name, tile):
    coords, conn, geom = mesh(name)[:3]
    lam, mu = Q.lame()
    lf = make_loss(tile_elems=tile)
    m = make_model(name, u=Q.patch_field(coords))
    loss, gx, gu = run_autograd(m, lf)
    want = Q.area(coords, conn) * Q.psi_of_F(Q.F0, lam, mu).item()
    assert abs(loss.item() - want) <= 1e-12 * abs(want)
    for g, which in ((gx, "x"), (gu, "u")):
        g = m.to_caller_order(g, which).cpu()
        assert g[~geom].abs().max() <= 1e-10 * g.abs().max()
    assert abs(lf.info[0].item() - torch.linalg.det(Q.F0).item()) <= 1e-13
    a = lf(make_model(name)).item()
    b = lf(make_model(name, u=Q.rotate_field(coords, Q.field(coords)))).item()
    assert abs(a - b) <= 1e-12 * abs(a)


# ---------------------------------------------------------------- 4. small strains: against the shipped linear kernel
@pytest.mark.parametrize("name", ["grid33", "mixed"])
def test_small_strain_consistency_with_the_linear_kernel(name):
    """eps = 1e-4, plane="stress", forces off: Quad4NeoHookeanLoss2D(eps u) / eps^2 (gradients: / eps^2 for x, / eps for u)
    against EnergyLoss2D(grad_convention="physical") on u.  Bound: TWICE the deviation the CPU statement shows against the
    oracle's linear physical QUAD4 energy on this mesh at this eps (computed here from quad4_hyper_reference and the oracle,
    never from the device); the factor 2 leaves room for both kernels' 1e-10 parity bands."""
    from hidenn_fem_amd.loss import EnergyLoss2D
    eps = 1e-4
    coords, conn = mesh(name)[:2]
    u = Q.field(coords)
    lam, mu = Q.lame()
    cpu = Q.total(coords, eps * u, conn, lam, mu)
    lin, lgx, lgu = Q.linear_physical(coords, u, conn)
    bound = (2 * abs(cpu["loss"] / eps ** 2 - lin) / abs(lin), 2 * ((cpu["gX"] / eps ** 2 - lgx).abs().max() / lgx.abs().max()).item(),
             2 * ((cpu["gU"] / eps - lgu).abs().max() / lgu.abs().max()).item())
    m_nh, m_lin = make_model(name, u=eps * u), make_model(name)
    nl, ngx, ngu = run_autograd(m_nh, make_loss())
    lin_fn = EnergyLoss2D(device=torch.device("cuda:0"), dtype=F64, grad_convention="physical")
    for p in (m_lin.node_coords_free, m_lin.u_free):
        p.grad = None
    ll = lin_fn(m_lin)
    ll.backward()
    lx, lu = m_lin.node_coords_free.grad, m_lin.u_free.grad
    got = (abs(nl.item() / eps ** 2 - ll.item()) / abs(ll.item()), ((ngx / eps ** 2 - lx).abs().max() / lx.abs().max()).item(),
           ((ngu / eps - lu).abs().max() / lu.abs().max()).item())
    print(name, "device deviation", got, "bound", bound)
    for g, b in zip(got, bound):
        assert 0 < b < 2e-4 and g <= b


# ---------------------------------------------------------------- 5. inversion rule
@pytest.mark.parametrize("name,tile", [("mixed", 0), ("plate", 64)], ids=["mixed-0", "plate-64"])
def test_inversion_rule(name, tile):
    coords, conn = mesh(name)[:2]
    v, node = Q.invert_one_cell(coords, Q.field(coords), conn)
    ref = reference(name, u=v, key="inverted")
    assert ref["count"] == 1 and ref["loss"] == float("inf") and ref["min_J"] < 0
    m, lf = make_model(name, u=v), make_loss(tile_elems=tile)
    loss, gx, gu = run_autograd(m, lf)
    assert loss.item() == float("inf") and lf.info[1].item() == 1.0
    assert torch.isfinite(gx).all() and torch.isfinite(gu).all()
    check(m, name, ref, loss, gx, gu, lf.info, what="inverted")          # the rows are the sum over the OTHER cells
    loss = lf.value_and_grad_(m)
    assert loss.item() == float("inf") and torch.isfinite(m.u_free.grad).all() and torch.isfinite(m.node_coords_free.grad).all()


# ---------------------------------------------------------------- 6. directional finite difference
@pytest.mark.parametrize("name,tile", [("mixed", 0), ("plate", 64)], ids=["mixed-0", "plate-64"])
def test_directional_finite_difference_on_the_device_alone(name, tile):
    """(Pi(p + h d) - Pi(p - h d)) / 2h against g . d for one random direction over both parameter sets, device numbers only.
    h: the LARGEST of 1e-3, 1e-4, 1e-5, 1e-6 at which the same quotient on the CPU statement is within 1e-6 |g . d| of the
    CPU g . d -- there the truncation term (the same on both sides) dominates the quotient's rounding; bound: twice that CPU
    error."""
    coords, conn, _, _, _, edges = mesh(name)
    mx, mu_ = masks(name)
    gen = torch.Generator().manual_seed(11)
    dX = torch.zeros_like(coords)
    dU = torch.zeros_like(coords)
    dX[mx] = 0.02 * (torch.rand(int(mx.sum()), 2, generator=gen, dtype=F64) - 0.5)
    dU[mu_] = 0.02 * (torch.rand(int(mu_.sum()), 2, generator=gen, dtype=F64) - 0.5)
    lam, mu = Q.lame()
    u = Q.field(coords)
    T = Q.traction_table(coords, edges) if name == "plate" else None     # default traction: constant, independent of x

    def cpu(h):
        return Q.total(coords + h * dX, u + h * dU, conn, lam, mu, None, edges if name == "plate" else None, T)

    r0 = cpu(0.0)
    gd = ((r0["gX"] * dX).sum() + (r0["gU"] * dU).sum()).item()
    h, bound = None, None
    for cand in (1e-3, 1e-4, 1e-5, 1e-6):
        err = abs((cpu(cand)["loss"] - cpu(-cand)["loss"]) / (2 * cand) - gd)
        if err <= 1e-6 * abs(gd):
            h, bound = cand, 2 * err
            break
    assert h is not None and bound > 0
    m, lf = make_model(name), make_loss(tile_elems=tile)
    _, gx, gu = run_autograd(m, lf)
    dx_s, du_s = m.from_caller_order(dX[mx], "x").cuda(), m.from_caller_order(dU[mu_], "u").cuda()
    g_dot_d = ((gx * dx_s).sum() + (gu * du_s).sum()).item()
    vals = []
    with torch.no_grad():
        x0, u0 = m.node_coords_free.clone(), m.u_free.clone()
        for sgn in (1.0, -1.0):
            m.node_coords_free.copy_(x0 + sgn * h * dx_s)
            m.u_free.copy_(u0 + sgn * h * du_s)
            vals.append(lf(m).item())
    q = (vals[0] - vals[1]) / (2 * h)
    print(name, "h", h, "device |q - g.d|", abs(q - g_dot_d), "bound", bound, "g.d", g_dot_d)
    assert abs(q - g_dot_d) <= bound


# ---------------------------------------------------------------- 7. plumbing
def test_two_calls_are_bitwise_equal_in_the_loss_and_info_is_one_tensor():
    from hidenn_fem_amd.loss import NeoHookeanLoss2D
    m, lf = make_model("plate"), make_loss(tile_elems=64)
    assert isinstance(lf, NeoHookeanLoss2D)
    a = lf(m).clone()
    info = lf.info
    b = lf(m)
    assert torch.equal(a, b) and lf.info is info
    c = lf.value_and_grad_(m)
    assert torch.equal(a, c) and lf.info is info and lf.value_and_grad_(m) is c
    assert info.dtype == F64 and info.shape == (2,) and info.is_cuda
    assert lf.lame == Q.lame() and lf.grad_convention == "physical"
    assert make_loss(plane="strain").lame == Q.lame(plane="strain")
    import src.loss
    assert src.loss.Quad4NeoHookeanLoss2D is type(lf)


def test_the_call_is_capturable():
    """One capture of ``value_and_grad_``, two replays after changing ``u_free`` in place: loss and gradients match uncaptured
    calls on a second model within the parity tolerances."""
    name = "plate"
    m, lf = make_model(name), make_loss(tile_elems=64)
    twin, lf2 = make_model(name), make_loss(tile_elems=64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lf.value_and_grad_(m)                                       # warm-up: plan, caches, .grad
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = lf.value_and_grad_(m)
    for factor in (0.9, 1.07):
        with torch.no_grad():
            m.u_free.mul_(factor)
            twin.u_free.mul_(factor)
            m.u_free.grad.zero_()
            m.node_coords_free.grad.zero_()
        graph.replay()
        want = lf2.value_and_grad_(twin)
        assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
        for p, q in ((m.u_free, twin.u_free), (m.node_coords_free, twin.node_coords_free)):
            assert (p.grad - q.grad).abs().max() <= 1e-10 * q.grad.abs().max() and q.grad.abs().max() > 0
        assert abs(lf.info[0].item() - lf2.info[0].item()) <= 1e-13 and lf.info[1].item() == 0


def test_fused_lbfgs_lowers_the_energy_from_the_linear_solution():
    """The plate (E = 2e6, so the default traction strains it by ~5 %) from its linear QUAD4 frozen-mesh solution: five
    FusedLBFGS steps on ``u_free`` lower the Neo-Hookean potential and invert nothing."""
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.optim import FusedLBFGS
    from hidenn_fem_amd.solve import solve_displacement_
    coords, conn, geom, bc, _, edges = mesh("plate")
    dev = torch.device("cuda:0")
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
    solve_displacement_(m, EnergyLoss2D(E=2e6, device=dev, dtype=F64, grad_convention="physical"), rtol=1e-10)
    lf = make_loss(E=2e6)
    start = lf.value_and_grad_(m).item()
    assert math.isfinite(start) and lf.info[1].item() == 0 and m.u_free.abs().max().item() > 0.05
    opt = FusedLBFGS([m.u_free])
    for _ in range(5):
        opt.step(lambda: lf.value_and_grad_(m))
        assert lf.info[1].item() == 0
    end = lf.value_and_grad_(m).item()
    print("Pi", start, "->", end, "min J", lf.info[0].item())
    assert end < start and lf.info[1].item() == 0


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.loss import Quad4NeoHookeanLoss2D
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.newton import newton_solve_
    from hidenn_fem_amd.plan import TilePlan, model_plan
    from hidenn_fem_amd.post import StressRecovery
    from hidenn_fem_amd.solve import Quad4FrozenMeshSolver, assemble_stiffness
    lf = make_loss()
    t = structured_tri_mesh(5, 4, dtype=F64)
    tri = PiecewiseLinearShapeNN2D(t[0], t[1]).to(torch.device("cuda:0"))
    for call in (lambda: lf(tri), lambda: lf.domain_energy(tri), lambda: lf.value_and_grad_(tri)):
        with pytest.raises(NotImplementedError):
            call()
    m = make_model("plate")
    for tool in (Quad4FrozenMeshSolver, assemble_stiffness, StressRecovery, newton_solve_):
        with pytest.raises(NotImplementedError):
            tool(m, lf)
    for kw in (dict(deterministic=True), dict(arithmetic="fp32")):
        with pytest.raises((ValueError, NotImplementedError)):
            Quad4NeoHookeanLoss2D(**kw)
    with pytest.raises(ValueError):
        Quad4NeoHookeanLoss2D(plane="axisymmetric")
    # the C entry point: an argument error (-1), never a launch; loss_out untouched
    plan, tri_plan = m.tile_plan(0), model_plan(tri, 0, paired=False)
    host = TilePlan(m.connectivity, m.Nnodes, coords_hint=m.initial_node_coords, x_src=m._x_src, u_src=m._u_src,
                    edges=m.neumann_edges, tile_elems=0, device=None, nodes_per_elem=4)
    x, u = m.node_coords_free.detach(), m.u_free.detach()
    xf, uf = m.node_coords_fixed.contiguous(), m.u_fixed_rows().contiguous()
    gx, gu = torch.zeros_like(x), torch.zeros_like(u)
    loss, work = torch.full((1,), 7.0, dtype=F64, device=x.device), torch.zeros(3 * 8, dtype=F64, device=x.device)
    lame, tc = (C.c_double * 2)(*lf.lame), (C.c_double * 4)(0, 0, 0, 0)

    def call(plan, flags, loss_t=loss, work_t=work, tconst=tc, gxp=gx):
        return _lib.lib().hfem_quad4_hyper_energy_plan(plan.handle, 0, x.data_ptr(), xf.data_ptr(), u.data_ptr(), uf.data_ptr(), lame,
                                                       None, None, tconst, None if loss_t is None else loss_t.data_ptr(), None,
                                                       None if work_t is None else work_t.data_ptr(),
                                                       None if gxp is None else gxp.data_ptr(), gu.data_ptr(), flags, None)

    err = lambda: _lib.lib().hfem_last_error().decode()
    assert call(tri_plan, 0) == -1 and "TRI3" in err()
    assert call(host, 0) == -1 and "host-only" in err()
    for flags in (64, 8, 128):
        assert call(plan, flags) == -1 and "flags" in err()
    assert call(plan, 0, None) == -1 and "null" in err()
    assert call(plan, 0, work_t=None) == -1 and "null" in err()
    assert call(plan, 0, gxp=None) == -1 and "gx_free" in err()
    assert call(plan, 0, tconst=None) == -1 and "traction" in err()
    host.close()
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and gx.abs().max().item() == 0.0      # nothing ran
    assert call(plan, 0) == 0
    torch.cuda.synchronize()
    assert loss.item() != 7.0
    assert call(plan, 4, tconst=None) == 0 and call(plan, 1, gxp=None) == 0      # edges off / no gx: the pointers may be NULL


def test_the_largest_tiles_run_and_a_tile_beyond_64_kib_of_lds_never_gets_a_plan():
    """40 x 40 nodes at tile_elems=4096: tiles of up to 939 local nodes and 863 slots (57 KiB of LDS; local ids and slots past
    768 in use) run and match the statement.  32 x 32 nodes in one tile would need 1024 local nodes, all owned -- 32 B per node
    + 32 B per owned row + 96 B = 65632 B: the planner refuses to build that device plan, so the entry point's own LDS check
    (the same sum) is a guard no device plan reaches."""
    from hidenn_fem_amd.mesh import structured_quad_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    dev = torch.device("cuda:0")
    lf = make_loss(tile_elems=4096)
    q = structured_quad_mesh(32, 32, dtype=F64)
    with pytest.raises(RuntimeError, match="LDS"):
        lf.value_and_grad_(PiecewiseLinearShapeNN2D(q[0], q[1]).to(dev))
    coords, conn = structured_quad_mesh(40, 40, dtype=F64)[:2]
    m = PiecewiseLinearShapeNN2D(coords, conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(Q.field(coords), "u"))
    m = m.to(dev)
    st = m.tile_plan(4096).stats
    assert st["max_tile_nodes"] > 768 and st["max_tile_elems"] > 768
    ref = Q.total(coords, Q.field(coords), conn, *Q.lame())
    loss = lf.value_and_grad_(m)
    gx = m.to_caller_order(m.node_coords_free.grad, "x").cpu()
    gu = m.to_caller_order(m.u_free.grad, "u").cpu()
    assert abs(loss.item() - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert (gx - ref["gX"]).abs().max() <= 1e-10 * ref["gX"].abs().max() and (gu - ref["gU"]).abs().max() <= 1e-10 * ref["gU"].abs().max()
    assert abs(lf.info[0].item() - ref["min_J"]) <= 1e-13 and lf.info[1].item() == 0
