"""Nodal stress recovery and the ZZ error estimate on the device (csrc/recover.hip, hidenn_fem_amd.post.StressRecovery)
against their CPU statement (tests/zz_reference.py, pinned on its own by tests/test_zz_reference_host.py), and the QUAD4
``von_mises``.  The field is u = 1e-4 (sin 2.1x cos 1.3y, 0.5 cos(1.7x + 0.3) sin 2.4y) interpolated at the nodes: no solve.

Tolerances are the project's parity tolerances -- the kernels and the reference differ in summation order and fma
contraction only: nodal stress 1e-11 max|sigma*|, eta_e^2 1e-10 max eta_e^2, the two totals 1e-11 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import quad_meshes as QM
import zz_reference as Z
from oracle import ref_chain as R

F64 = torch.float64
pytestmark = pytest.mark.gpu
MESHES = ["tri_structured", "tri_unstructured", "quad_structured", "quad_split", "quad_split_renumbered"]
CONVENTIONS = ["reference", "physical"]

_cache = {}


def mesh(name):
    if "meshes" not in _cache:
        _cache["meshes"] = Z.meshes()
    return _cache["meshes"][name]


def reference(name, conv, fld="field"):
    """The CPU result of one (mesh, convention, field): computed once, shared, never modified."""
    key = (name, conv, fld)
    if key not in _cache:
        coords, conn = mesh(name)[:2]
        u = getattr(Z, fld)(coords)
        Cm = R.plane_stress_C()
        r = Z.zz(coords, u, conn, Cm, conv)
        r["area"] = Z.recover(coords, u, conn, Cm, conv)[1]
        _cache[key] = r
    return _cache[key]


def make_model(name, fld="field", dtype=F64):
    """Every node free, no Neumann edges; u_full = the field at the nodes."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    coords, conn = mesh(name)[:2]
    m = PiecewiseLinearShapeNN2D(coords.to(dtype), conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(getattr(Z, fld)(coords).to(dtype), "u"))
    return m.to(torch.device("cuda:0"))


def make_loss(conv, dtype=F64, **kw):
    from hidenn_fem_amd.loss import EnergyLoss2D
    return EnergyLoss2D(device=torch.device("cuda:0"), dtype=dtype, grad_convention=conv, **kw)


def rel_max(got, ref):
    ref = ref if torch.is_tensor(ref) else torch.as_tensor(ref)
    return ((got.detach().cpu().double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("conv", CONVENTIONS)
@pytest.mark.parametrize("name", MESHES)
def test_parity_with_the_cpu_statement(name, conv):
    from hidenn_fem_amd.post import StressRecovery
    ref = reference(name, conv)
    m = make_model(name)
    sr = StressRecovery(m, make_loss(conv))
    sig, area = sr.nodal_stress(return_area=True)
    err = sr.error()
    figures = dict(sigma=rel_max(sig, ref["nodal_stress"]), area=rel_max(area, ref["area"]), eta2=rel_max(err.eta2, ref["eta2"]),
                   norm2=abs(err.energy_norm2 - ref["norm2_total"]) / ref["norm2_total"], eta=abs(err.eta - ref["eta"]) / ref["eta"],
                   rel=abs(err.relative - ref["relative"]) / ref["relative"])
    print(name, conv, {k: f"{v:.2e}" for k, v in figures.items()}, f"eta_rel {err.relative:.4f}")
    assert sig.shape == (m.Nnodes, 3) and err.eta2.shape == (m.Nelems,) and sig.dtype == F64 and err.eta2.dtype == F64
    assert figures["sigma"] <= 1e-11 and figures["area"] <= 1e-11
    assert figures["eta2"] <= 1e-10
    assert figures["norm2"] <= 1e-11 and figures["eta"] <= 1e-11 and figures["rel"] <= 1e-11
    assert torch.equal(err.nodal_stress, sig)
    # the totals are the sums of the per-element arrays, and relative is what the issue defines
    assert abs(err.eta ** 2 - err.eta2.sum().item()) <= 1e-12 * err.eta ** 2
    assert abs(err.relative - (err.eta ** 2 / (err.energy_norm2 + err.eta ** 2)) ** 0.5) <= 1e-15
    s = ref["nodal_stress"]
    vm = torch.sqrt(s[:, 0] ** 2 - s[:, 0] * s[:, 1] + s[:, 1] ** 2 + 3.0 * s[:, 2] ** 2)
    assert rel_max(sr.nodal_von_mises(), vm) <= 1e-11


@pytest.mark.parametrize("name", MESHES)
def test_patch_test_physical_convention(name):
    """A linear field has a constant stress: sigma* = sigma_h and eta = 0 up to rounding (the CPU statement: < 3e-15)."""
    from hidenn_fem_amd.post import zz_error
    err = zz_error(make_model(name, "linear_field"), make_loss("physical"))
    print(name, f"eta_rel {err.relative:.3e} (reference {reference(name, 'physical', 'linear_field')['relative']:.3e})")
    assert err.relative <= 1e-12
    assert err.energy_norm2 > 0.0


@pytest.mark.parametrize("conv", CONVENTIONS)
@pytest.mark.parametrize("name", ["tri_structured", "tri_unstructured", "quad_structured", "quad_split"])
def test_energy_norm_is_twice_the_strain_energy(name, conv):
    """No Neumann edges, default (zero) body force: the loss is the strain energy sum |det| W psi, and
    ||u_h||^2 = sum w sigma.S.sigma = 2 x strain energy.  TRI3: with a rule whose weights sum to 1/2 (order 1, the default
    of ``triangle_gauss_points``) W |det| = A; EnergyLoss2D's own default, order 4, carries the reference's extra 0.5
    (weights sum to 1/4), so its value is half the strain energy and the factor is 4."""
    from hidenn_fem_amd.post import zz_error
    m = make_model(name)
    quad = mesh(name)[1].shape[1] == 4
    loss_fn = make_loss(conv) if quad else make_loss(conv, gauss_order=1)
    n2 = zz_error(m, loss_fn).energy_norm2
    e = loss_fn(m).item()
    print(name, conv, f"norm2 {n2:.15e} 2E {2 * e:.15e} rel {abs(n2 - 2 * e) / (2 * e):.2e}")
    assert abs(n2 - 2.0 * e) <= 1e-11 * 2.0 * e
    if not quad:
        e4 = make_loss(conv)(m).item()
        assert abs(n2 - 4.0 * e4) <= 1e-11 * n2


@pytest.mark.parametrize("name", ["tri_unstructured", "quad_split_renumbered"])
def test_two_calls_are_bitwise_equal(name):
    from hidenn_fem_amd.post import StressRecovery
    m = make_model(name)
    for conv in CONVENTIONS:
        sr = StressRecovery(m, make_loss(conv))
        s1, a1 = sr.nodal_stress(return_area=True)
        e1 = sr.error()
        s2, a2 = StressRecovery(m, make_loss(conv)).nodal_stress(return_area=True)
        e2 = sr.error()
        assert torch.equal(s1, s2) and torch.equal(a1, a2) and torch.equal(e1.eta2, e2.eta2)
        assert torch.equal(e1.nodal_stress, s1) and torch.equal(e2.nodal_stress, s1)
        assert (e1.energy_norm2, e1.eta, e1.relative) == (e2.energy_norm2, e2.eta, e2.relative)


def test_renumbered_mesh_maps_back_to_the_original():
    """Cell order, node ids, starting corners and orientations changed: in the physical convention the recovered field is the
    same field (a_old[old_of_new] = a_new) and the totals are the same numbers, up to the summation order."""
    from hidenn_fem_amd.post import StressRecovery
    _, old_of_new = QM.renumber(mesh("quad_split"), seed=5, orient="mixed")
    assert torch.equal(mesh("quad_split")[0][old_of_new], mesh("quad_split_renumbered")[0])
    a = StressRecovery(make_model("quad_split"), make_loss("physical")).error()
    b = StressRecovery(make_model("quad_split_renumbered"), make_loss("physical")).error()
    back = torch.empty_like(a.nodal_stress)
    back[old_of_new.to(back.device)] = b.nodal_stress
    fig = dict(sigma=rel_max(back, a.nodal_stress.cpu()), norm2=abs(a.energy_norm2 - b.energy_norm2) / a.energy_norm2,
               eta=abs(a.eta - b.eta) / a.eta)
    print({k: f"{v:.2e}" for k, v in fig.items()})
    assert fig["sigma"] <= 1e-11 and fig["norm2"] <= 1e-11 and fig["eta"] <= 1e-11
    assert abs(np.sort(a.eta2.cpu().numpy()) - np.sort(b.eta2.cpu().numpy())).max() <= 1e-10 * a.eta2.max().item()


def test_stays_valid_when_the_nodes_move_and_skips_unreferenced_nodes():
    """One object across coordinate updates (the connectivity never changes); a node of no element gets zeros."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.post import StressRecovery
    coords, conn = mesh("tri_structured")[:2]
    extra = torch.cat([coords, torch.tensor([[9.0, 9.0]], dtype=F64)])
    m = PiecewiseLinearShapeNN2D(extra, conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(Z.field(extra), "u"))
    m = m.to(torch.device("cuda:0"))
    sr = StressRecovery(m, make_loss("physical"))
    sig, area = sr.nodal_stress(return_area=True)
    assert sig[-1].abs().max().item() == 0.0 and area[-1].item() == 0.0
    assert rel_max(sig[:-1], reference("tri_structured", "physical")["nodal_stress"]) <= 1e-11
    g = torch.Generator().manual_seed(4)
    moved = extra + 0.004 * (torch.rand(extra.shape, generator=g, dtype=F64) - 0.5)
    with torch.no_grad():
        m.node_coords_free.copy_(m.from_caller_order(moved, "x").to(m.device))
    ref = Z.zz(moved[:-1], Z.field(extra)[:-1], conn, R.plane_stress_C(), "physical")
    err = sr.error()
    assert rel_max(err.nodal_stress[:-1], ref["nodal_stress"]) <= 1e-11 and rel_max(err.eta2, ref["eta2"]) <= 1e-10


def test_quad4_von_mises_matches_the_centre_point_chain():
    from hidenn_fem_amd.post import von_mises
    for name in ("quad_structured", "quad_split_renumbered"):
        coords, conn = mesh(name)[:2]
        m = make_model(name)
        vm, gu = von_mises(m, return_grad_u=True)
        ref, g = Z.von_mises_centre(coords, Z.field(coords), conn)
        assert vm.shape == (m.Nelems,) and gu.shape == (m.Nelems, 2, 2)
        np.testing.assert_allclose(gu.cpu().numpy(), g, rtol=1e-12, atol=1e-16)
        np.testing.assert_allclose(vm.cpu().numpy(), ref, rtol=1e-12)
        assert torch.equal(von_mises(m), vm)


def test_tri3_von_mises_is_unchanged():
    """Bitwise against the call ``von_mises`` made before it learnt QUAD4, restated here on the same model."""
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.post import von_mises
    m = make_model("tri_structured")
    X, U = m.coords.detach(), m.u_full.detach()
    X64, U64 = X.to(F64).contiguous(), U.to(F64).contiguous()
    ne = m.Nelems
    vm = torch.empty(ne, dtype=F64, device=X.device)
    gu = torch.empty(ne, 2, 2, dtype=F64, device=X.device)
    _lib.check(_lib.lib().hfem_tri3_von_mises(_lib.dev_index(X.device), _lib.ptr(X64), _lib.ptr(U64), _lib.ptr(m._conn32), ne,
                                              10e9, 0.3, _lib.ptr(vm), _lib.ptr(gu), _lib.stream_ptr(X.device)))
    got_vm, got_gu = von_mises(m, return_grad_u=True)
    assert torch.equal(got_vm, vm) and torch.equal(got_gu, gu)


def test_edge_cases_of_the_c_abi():
    from hidenn_fem_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(torch.device("cuda:0"))
    mat = (C.c_double * 4)(*make_loss("reference")._mat)
    z = torch.zeros(64, dtype=F64, device="cuda:0")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p, pi = z.data_ptr(), zi.data_ptr()
    for kind in ("tri3", "quad4"):
        rec, zz = getattr(L, f"hfem_{kind}_stress_recover"), getattr(L, f"hfem_{kind}_zz_error")
        # zero sizes: 0, nothing touched
        assert rec(0, None, None, None, 0, 5, None, None, None, 0, None, None, st) == 0
        assert rec(0, None, None, None, 5, 0, None, None, None, 0, None, None, st) == 0
        assert zz(0, None, None, None, 0, None, None, 0, None, None, None, None, st) == 0
        # a null output pointer, a negative count, an unknown flag: a negative code and a message
        assert rec(0, p, p, pi, 1, 4, pi, pi, mat, 0, None, None, st) < 0 and b"null pointer" in L.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, mat, 0, None, None, p, p, st) < 0 and b"null pointer" in L.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, mat, 0, p, None, None, p, st) < 0 and b"null pointer" in L.hfem_last_error()
        assert rec(0, p, p, pi, -1, 4, pi, pi, mat, 0, p, None, st) < 0 and b"negative" in L.hfem_last_error()
        assert zz(0, p, p, pi, -1, p, mat, 0, p, None, p, p, st) < 0 and b"negative" in L.hfem_last_error()
        assert rec(0, p, p, pi, 1, 4, pi, pi, mat, 128, p, None, st) < 0 and b"flags" in L.hfem_last_error()
        assert rec(0, p, p, pi, 1 << 29, 4, pi, pi, mat, 0, p, None, st) < 0 and b"2^29" in L.hfem_last_error()
    assert L.hfem_quad4_von_mises(0, None, None, None, 0, 1e9, 0.3, None, None, st) == 0
    assert L.hfem_quad4_von_mises(0, p, p, pi, 1, 1e9, 0.3, None, None, st) < 0 and b"null pointer" in L.hfem_last_error()
    assert L.hfem_quad4_von_mises(0, p, p, pi, -1, 1e9, 0.3, p, None, st) < 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["tri_structured", "quad_structured"])
def test_fp32_models_get_fp32_results(name):
    """Widened on the way in, computed in fp64, rounded once on the way out."""
    from hidenn_fem_amd.post import StressRecovery, recover_stress, von_mises
    m = make_model(name, dtype=torch.float32)
    loss_fn = make_loss("physical", dtype=torch.float32)
    sr = StressRecovery(m, loss_fn)
    err = sr.error()
    assert err.eta2.dtype == torch.float32 and err.nodal_stress.dtype == torch.float32
    assert sr.nodal_stress().dtype == torch.float32 and sr.nodal_von_mises().dtype == torch.float32
    assert recover_stress(m, loss_fn).dtype == torch.float32 and von_mises(m).dtype == torch.float32
    assert isinstance(err.eta, float) and 0.0 < err.relative < 1.0
    # the fp32 inputs are the fp64 ones rounded (2^-24 relative): a difference quotient over h ~ length / 22 of coordinates up
    # to 2 loses a factor ~ 2 / h ~ 25, squared quantities double it -- ~ 3e-6; 1e-4 leaves room and still tells fp64 maths
    ref = reference(name, "physical")
    assert abs(err.energy_norm2 - ref["norm2_total"]) <= 1e-4 * ref["norm2_total"]
