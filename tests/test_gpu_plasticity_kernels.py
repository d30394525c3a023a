"""The J2 elastoplastic kernels on the device (csrc/tri3_j2.hip, csrc/hfem_j2_dev.h, the J2 operator kind of csrc/cg.hip)
against their numpy statement (tests/plasticity_reference.py, pinned on its own by tests/test_plasticity_reference_host.py).

Meshes: the cases of tests/test_gpu_newton.py -- the jittered and the Delaunay mesh (every row free), the 17 x 9 plate (free and
fixed rows mixed, Neumann edges) at the default tile size and at tile_elems=64, and the jittered mesh with every element listed
ten times at tile_elems=4096 (one tile of 2560 slots: the loop behind the prefetched records).  Inputs: a random committed state
and a displacement field scaled so that the reference classifies 20-80 % of the elements plastic with none within 1e-6
(relative) of the yield surface -- both asserted on the reference inputs.  Tolerances: Pi 1e-12 relative; g 1e-10 max|g|; trial
state and stress 1e-12 max; plastic count exact; apply and diagonal blocks 1e-10 max against the dense K_T; p^T q within
1e-10 sum|p_i q_i|."""
import numpy as np
import pytest
import torch

import hyper_reference as H
import plasticity_reference as P
from oracle import ref_chain as R

F64, F32 = torch.float64, torch.float32
pytestmark = pytest.mark.gpu
CASES = [("jittered", 0), ("delaunay", 0), ("plate", 0), ("plate", 64), ("jittered_x10", 4096)]
IDS = [f"{n}-{t}" for n, t in CASES]
MAT = P.Material(E=10e9, nu=0.3, sigma_y=1e5, H=5e8)
_cache = {}


def dev():
    return torch.device("cuda:0")


def mesh(name):
    if "meshes" not in _cache:
        ms = H.meshes()
        j = ms["jittered"]
        ms["jittered_x10"] = (j[0], j[1].repeat(10, 1)) + tuple(j[2:])
        _cache["meshes"] = ms
    return _cache["meshes"][name]


def case(name, dtype=F64):
    """-> dict(prob, u [Nn, 2] node order, ep, al, load 1 quantities of the reference), computed once per (mesh, dtype)."""
    key = (name, dtype)
    if key in _cache:
        return _cache[key]
    c0, conn, geom, bc, _, edges = mesh(name)
    coords = c0.to(dtype).to(F64).numpy()
    W = float(R.triangle_gauss(4, dtype)[1].to(F64).sum())
    plate = name == "plate"
    bcn = bc.numpy() if plate else np.zeros(coords.shape[0], dtype=bool)
    rng = np.random.default_rng(11)
    ne = conn.shape[0]
    radius = P.RT23 * MAT.sigma_y / (2 * MAT.mu)                       # the yield strain
    m0 = P.Mesh(coords, conn.numpy(), W)
    e0 = m0.strain(H.field(c0).numpy())
    tr = e0[:, 0] + e0[:, 1]
    dn = np.sqrt((e0[:, 0] - tr / 3) ** 2 + (e0[:, 1] - tr / 3) ** 2 + (tr / 3) ** 2 + 2 * e0[:, 2] ** 2)
    u = (H.field(c0) * (radius / np.median(dn))).to(dtype).to(F64).numpy()
    ep = rng.normal(size=(ne, 3)) * 0.15 * radius
    al = np.abs(rng.normal(size=ne)) * 2e-5
    f_ext = P.edge_loads(coords, edges.numpy(), (100e3, 0.0)) if plate else None      # the loss's default traction
    prob = P.Problem(coords, conn.numpy(), bcn, MAT, W, u[bcn], f_ext)
    uf = u[~bcn]
    Pi, g, r = prob.energy(uf, ep, al, 1.0)
    frac = r["plastic"].mean()
    margin = np.abs(r["f"]).min() / (P.RT23 * MAT.sigma_y)
    print(name, dtype, "plastic fraction", frac, "closest to the yield surface", margin)
    assert 0.2 <= frac <= 0.8 and margin >= 1e-6
    _cache[key] = dict(prob=prob, u=u, uf=uf, ep=ep, al=al, Pi=Pi, g=g, r=r, bc=bcn, K=prob.tangent(uf, ep, al, 1.0))
    return _cache[key]


def make_model(name, u, dtype=F64):
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    c0, conn, geom, bc, _, edges = mesh(name)
    u = torch.as_tensor(u)
    if name == "plate":
        m = PiecewiseLinearShapeNN2D(c0.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=u[bc].to(dtype),
                                     neumann_edges=edges)
        free_u = u[~bc]
    else:
        m = PiecewiseLinearShapeNN2D(c0.to(dtype), conn)
        free_u = u
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(free_u.to(dtype), "u"))
    return m.to(dev())


def make_solver(name, tile, dtype=F64, **kw):
    from hidenn_fem_amd.plasticity import ElastoplasticSolver, J2PlasticityLoss2D
    c = case(name, dtype)
    m = make_model(name, c["u"], dtype)
    lf = J2PlasticityLoss2D(E=MAT.E, nu=MAT.nu, sigma_y=MAT.sigma_y, hardening=MAT.H, device=dev(), dtype=dtype, tile_elems=tile)
    s = ElastoplasticSolver(m, lf, **kw)
    s.set_state(torch.as_tensor(c["ep"]), torch.as_tensor(c["al"]))
    return c, m, s


def to_dev(m, rows):
    return m.from_caller_order(torch.as_tensor(rows), "u").to(dev()).contiguous()


def to_ref(m, rows):
    return m.to_caller_order(rows.detach(), "u").cpu().double().numpy()


def random_p(n, seed=5):
    return (torch.rand(n, 2, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 0.5).numpy()


def check_update(c, m, s, what):
    out, g = s.evaluate()
    out = out.tolist()
    g = to_ref(m, g)
    ep, al = s.state(trial=True)
    sig = s.stress().cpu().numpy()
    r = c["r"]
    e_pi = abs(out[0] - c["Pi"]) / abs(c["Pi"])
    e_g = np.abs(g - c["g"]).max() / np.abs(c["g"]).max()
    e_ep = np.abs(ep.cpu().numpy() - r["ep"]).max() / np.abs(r["ep"]).max()
    e_al = np.abs(al.cpu().numpy() - r["al"]).max() / np.abs(r["al"]).max()
    e_s = np.abs(sig - r["sig"]).max() / np.abs(r["sig"]).max()
    e_dg = abs(out[2] - r["dgamma"].max()) / r["dgamma"].max()
    print(what, "Pi", f"{e_pi:.2e}", "g", f"{e_g:.2e}", "eps_p", f"{e_ep:.2e}", "alpha", f"{e_al:.2e}", "stress", f"{e_s:.2e}",
          "max dgamma", f"{e_dg:.2e}", "plastic", out[1], int(r["plastic"].sum()))
    assert e_pi <= 1e-12 and e_g <= 1e-10
    assert e_ep <= 1e-12 and e_al <= 1e-12 and e_s <= 1e-12 and e_dg <= 1e-12
    assert out[1] == float(r["plastic"].sum())
    assert abs(s.plastic_fraction) == 0.0                              # no solve yet: evaluate() is not a step
    vm = s.von_mises().cpu().numpy()
    assert np.abs(vm - P.von_mises(r["sig"])).max() <= 1e-12 * np.abs(r["sig"]).max()


# ---------------------------------------------------------------- 1. update launch
@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_update_equals_the_reference(name, tile):
    c, m, s = make_solver(name, tile)
    before = s.state()
    check_update(c, m, s, f"{name}-{tile}")
    after = s.state()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])       # an update never writes the committed state
    assert torch.equal(before[0].cpu(), torch.as_tensor(c["ep"])) and torch.equal(before[1].cpu(), torch.as_tensor(c["al"]))
    # bit-identical state and stress across repeats
    t1, s1 = s.state(trial=True), s.stress()
    s.evaluate()
    t2, s2 = s.state(trial=True), s.stress()
    assert torch.equal(t1[0], t2[0]) and torch.equal(t1[1], t2[1]) and torch.equal(s1, s2)


def test_update_of_an_fp32_model():
    c, m, s = make_solver("plate", 64, F32)
    assert m.u_free.dtype == F32
    check_update(c, m, s, "plate-64 fp32")


def test_update_commit_update_at_the_same_u():
    c, m, s = make_solver("plate", 64)
    _, g1 = s.evaluate()
    ep1, al1 = s.state(trial=True)
    s.commit()
    ep_c, al_c = s.state()
    assert torch.equal(ep_c, ep1) and torch.equal(al_c, al1)
    out2, g2 = s.evaluate()
    ep2, al2 = s.state(trial=True)
    d_ep = ((ep2 - ep1).abs().max() / ep1.abs().max()).item()
    d_al = ((al2 - al1).abs().max() / al1.abs().max()).item()
    d_g = ((g2 - g1).abs().max() / g1.abs().max()).item()
    print("state moved by", d_ep, d_al, "g by", d_g, "max dgamma", out2[2].item())
    assert d_ep <= 1e-12 and d_al <= 1e-12 and d_g <= 1e-10


# ---------------------------------------------------------------- 2. linearisation and apply
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,tile", CASES, ids=IDS)
def test_apply_and_diag_equal_the_dense_tangent(name, tile, dtype):
    c, m, s = make_solver(name, tile, dtype)
    K = c["K"]
    s._tan.fill_(float("nan"))                                         # records of padded and skipped slots stay NaN
    p = random_p(K.shape[0] // 2)
    q, pq = s.apply(to_dev(m, p))
    left = int(torch.isnan(s._tan).sum().item())
    assert torch.isfinite(q).all() and np.isfinite(pq.item())
    q = to_ref(m, q)
    want = (K @ p.reshape(-1)).reshape(-1, 2)
    e_q = np.abs(q - want).max() / np.abs(want).max()
    e_pq = abs(pq.item() - (p * want).sum()) / np.abs(p * want).sum()
    blocks = P.diag_blocks(K)
    e_d = np.abs(to_ref(m, s.diag) - blocks).max() / np.abs(blocks).max()
    print(name, tile, dtype, "q", f"{e_q:.2e}", "p^T q", f"{e_pq:.2e}", "diag", f"{e_d:.2e}", "NaN records left", left,
          "of", s._tan.numel())
    assert e_q <= 1e-10 and e_pq <= 1e-10 and e_d <= 1e-10
    assert s.info[0].item() == float(c["r"]["plastic"].sum()) and s.info[1].item() == 0.0
    if tile == 64:
        assert left > 0                                                # this plan has padded slots: the poison was live


# ---------------------------------------------------------------- 3. a captured graph survives a re-linearisation
def test_captured_iterate_graph_after_a_relinearisation_into_the_same_buffers():
    from hidenn_fem_amd import _lib
    c, m, s = make_solver("plate", 0, iters_per_graph=5)
    g = to_dev(m, random_p(s.n_u, seed=13))
    stream = _lib.stream_ptr(dev())

    def run(replay):
        s._g.copy_(g)
        s._delta.zero_()
        _lib.check(_lib.lib().hfem_cg_start(s._h, s._g.data_ptr(), s._g.data_ptr(), 1e-30, 0.0, 1000, stream), "hfem_cg_start")
        torch.cuda.synchronize()
        s._replay() if replay else s._iterate()
        st = s._read_status()
        assert st[0] == 5.0 and st[10] == 0.0
        return s._delta.clone()

    s.apply(g)                                                         # refresh + linearise at the case's u
    first = run(True)                                                  # captures the graph
    with torch.no_grad():
        m.u_free.mul_(0.4)                                             # another linearisation point: mostly elastic
    tan_ptr = s._tan.data_ptr()
    s.apply(g)
    assert s._tan.data_ptr() == tan_ptr and s.info[0].item() < float(c["r"]["plastic"].sum())
    graph, eager = run(True), run(False)
    err = ((graph - eager).abs().max() / eager.abs().max()).item()
    moved = ((graph - first).abs().max() / first.abs().max()).item()
    print("graph vs eager", err, "against the first linearisation", moved)
    assert err <= 1e-10 and moved > 1e-3
