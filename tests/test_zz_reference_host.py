"""The CPU statement of the stress recovery and the ZZ estimate (tests/zz_reference.py) pinned by what it must satisfy on
its own -- patch test, closed form against quadrature, convergence rate, invariance to the numbering -- and the host half of
the feature, ``hidenn_fem_amd.post.node_adjacency``.  No GPU."""
import numpy as np
import pytest
import torch

import quad_meshes as QM
import zz_reference as Z
from oracle import ref_chain as R

F64 = torch.float64


@pytest.fixture(scope="module")
def meshes():
    return Z.meshes()


@pytest.fixture(scope="module")
def C():
    return R.plane_stress_C()


def test_the_meshes_are_the_ones_the_tests_count_on(meshes):
    """More than one 256-thread block, no multiple of 256, fans from 1 to 10."""
    sizes = {k: (m[0].shape[0], m[1].shape[0]) for k, m in meshes.items()}
    assert sizes["tri_structured"] == (391, 704) and sizes["quad_structured"] == (437, 396)
    for k, (nn, ne) in sizes.items():
        assert nn > 256 and ne > 256 and nn % 256 and ne % 256, (k, nn, ne)
    val = {k: QM.valence(m[1].numpy(), m[0].shape[0]) for k, m in meshes.items()}
    assert (val["tri_structured"].min(), val["tri_structured"].max()) == (1, 6)
    assert val["tri_unstructured"].min() == 1 and val["tri_unstructured"].max() >= 8
    assert val["quad_split"].min() == 1 and val["quad_split"].max() >= 9


def test_patch_test_linear_field_physical_convention(meshes, C):
    for name, (coords, conn, *_) in meshes.items():
        r = Z.zz(coords, Z.linear_field(coords), conn, C, "physical")
        print(f"{name}: eta_rel {r['relative']:.3e}")
        assert r["relative"] <= 1e-13, (name, r["relative"])


def test_reference_convention_does_not_pass_the_patch_test(meshes, C):
    """Why the docstrings say that eta estimates the discretisation error only in the physical convention."""
    coords, conn = meshes["tri_structured"][:2]
    assert Z.zz(coords, Z.linear_field(coords), conn, C, "reference")["relative"] > 0.1


def test_tri3_closed_form_equals_three_point_quadrature(meshes, C):
    for name in ("tri_structured", "tri_unstructured"):
        coords, conn = meshes[name][:2]
        for conv in ("reference", "physical"):
            a = Z.zz(coords, Z.field(coords), conn, C, conv)["eta2"]
            b = Z.zz(coords, Z.field(coords), conn, C, conv, tri_rule="quad3")["eta2"]
            assert (a - b).abs().max().item() <= 1e-13 * b.max().item(), (name, conv)


@pytest.mark.parametrize("kind", ["tri", "quad"])
@pytest.mark.parametrize("jitter", [0.0, 0.2])
def test_eta_halves_twice_per_refinement(kind, jitter, C):
    """eta = O(h) with superconvergent recovery O(h^2) on these smooth fields: eta(n) / eta(2n - 1) ~ 2."""
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    mesher = structured_tri_mesh if kind == "tri" else structured_quad_mesh

    def eta(n):
        coords, conn = mesher(n, n, jitter=jitter, seed=1, dtype=F64)[:2]
        return Z.zz(coords, Z.field(coords), conn, C, "physical")["eta"]

    for n in (9, 17, 33):
        ratio = eta(n) / eta(2 * n - 1)
        print(f"{kind} jitter {jitter} n {n}: eta(n)/eta(2n-1) = {ratio:.4f}")
        assert 1.9 <= ratio <= 2.15, (kind, jitter, n, ratio)


def test_renumbering_leaves_eta_unchanged(meshes, C):
    a, b = meshes["quad_split"], meshes["quad_split_renumbered"]
    for conv in ("physical",):          # the reference convention depends on the local node order by construction
        ra = Z.zz(a[0], Z.field(a[0]), a[1], C, conv)
        rb = Z.zz(b[0], Z.field(b[0]), b[1], C, conv)
        assert abs(ra["eta2_total"] - rb["eta2_total"]) <= 1e-13 * ra["eta2_total"]
        assert abs(ra["norm2_total"] - rb["norm2_total"]) <= 1e-13 * ra["norm2_total"]


def test_lumped_areas_add_up_to_the_domain(meshes, C):
    for name, (coords, conn, *_) in meshes.items():
        _, den = Z.recover(coords, Z.field(coords), conn, C)
        pts, wf = Z.points(conn.shape[1])
        _, adet = Z.point_stress(coords, Z.field(coords), conn, C, "reference", pts)
        assert abs(den.sum().item() - (adet * wf).sum().item()) <= 1e-13 * den.sum().item(), name


# ---------------------------------------------------------------- node_adjacency (the host half of the feature)
def test_node_adjacency_lists_every_corner_once_in_ascending_element_order(meshes):
    from hidenn_fem_amd.post import node_adjacency
    for name, (coords, conn, *_) in meshes.items():
        nn, (ne, npe) = coords.shape[0], conn.shape
        adj_ptr, adj = node_adjacency(conn, nn)
        assert adj_ptr.dtype == torch.int32 and adj.dtype == torch.int32 and adj_ptr.device.type == "cpu"
        assert adj_ptr.shape == (nn + 1,) and adj.shape == (npe * ne,)
        p, a = adj_ptr.numpy().astype(np.int64), adj.numpy().astype(np.int64)
        assert p[0] == 0 and p[-1] == npe * ne
        np.testing.assert_array_equal(np.diff(p), QM.valence(conn.numpy(), nn))
        e, c = a >> 2, a & 3
        assert c.max() < npe
        np.testing.assert_array_equal(np.sort(e * npe + c), np.arange(npe * ne))       # every (element, corner) exactly once
        node_of = np.repeat(np.arange(nn), np.diff(p))
        np.testing.assert_array_equal(conn.numpy()[e, c], node_of)                      # ... and under its own node
        same = node_of[1:] == node_of[:-1]
        assert (np.diff(e)[same] > 0).all(), name                                       # ascending element id at each node


def test_node_adjacency_accepts_int32_and_rejects_bad_input():
    from hidenn_fem_amd.post import node_adjacency
    conn = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    adj_ptr, adj = node_adjacency(conn, 5)                                               # node 4: in no element
    assert adj_ptr.tolist() == [0, 1, 3, 5, 6, 6]
    assert adj.tolist() == [0 << 2 | 0, 0 << 2 | 1, 1 << 2 | 1, 0 << 2 | 2, 1 << 2 | 0, 1 << 2 | 2]
    with pytest.raises(ValueError, match="out of range"):
        node_adjacency(conn, 3)


def test_node_adjacency_raises_at_the_packing_limit():
    """e << 2 | c must fit int32: Ne < 2**29.  A stubbed shape, not a real allocation."""
    from hidenn_fem_amd.post import node_adjacency

    class Stub:
        def __init__(self, ne):
            self.shape = (ne, 3)

    with pytest.raises(ValueError, match=r"2\*\*29"):
        node_adjacency(Stub(2 ** 29), 10)
    with pytest.raises(ValueError, match=r"2\*\*29"):
        node_adjacency(Stub(2 ** 29 + 5), 10)


# ---------------------------------------------------------------- the C ABI's argument checks (no device is touched)
NEW_SYMBOLS = ["hfem_tri3_stress_recover", "hfem_quad4_stress_recover", "hfem_tri3_zz_error", "hfem_quad4_zz_error",
               "hfem_quad4_von_mises"]


def test_new_symbols_are_exported_and_bound_and_check_their_arguments_first():
    import ctypes as C
    from hidenn_fem_amd import _lib as L
    from hidenn_fem_amd.csrc import build
    build.build()
    h = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
    for kind in ("stress_recover", "zz_error"):
        assert L.PROTOTYPES[f"hfem_quad4_{kind}"] == L.PROTOTYPES[f"hfem_tri3_{kind}"]
    assert L.PROTOTYPES["hfem_quad4_von_mises"] == L.PROTOTYPES["hfem_tri3_von_mises"]
    lib = L.lib()
    buf = (C.c_double * 16)()
    ibuf = (C.c_int32 * 16)()
    p, pi = C.addressof(buf), C.addressof(ibuf)            # never dereferenced: every call below returns before a launch
    mat = (C.c_double * 4)(1.0, 0.3, 1.0, 0.35)
    for kind in ("tri3", "quad4"):
        rec, zz = getattr(lib, f"hfem_{kind}_stress_recover"), getattr(lib, f"hfem_{kind}_zz_error")
        assert rec(-7, None, None, None, 0, 5, None, None, None, 0, None, None, None) == 0          # not even the device id is read
        assert rec(-7, None, None, None, 5, 0, None, None, None, 0, None, None, None) == 0
        assert zz(-7, None, None, None, 0, None, None, 0, None, None, None, None, None) == 0
        assert rec(0, p, p, pi, 1, 4, pi, pi, mat, 0, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, mat, 0, None, None, p, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, mat, 0, p, None, p, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert rec(0, p, p, pi, -1, 4, pi, pi, mat, 0, p, None, None) < 0 and b"negative" in lib.hfem_last_error()
        assert rec(0, p, p, pi, 1, -4, pi, pi, mat, 0, p, None, None) < 0 and b"negative" in lib.hfem_last_error()
        assert zz(0, p, p, pi, -1, p, mat, 0, p, None, p, p, None) < 0 and b"negative" in lib.hfem_last_error()
        assert rec(0, p, p, pi, 1, 4, pi, pi, mat, 128, p, None, None) < 0 and b"flags" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, mat, 2, p, None, p, p, None) < 0 and b"flags" in lib.hfem_last_error()
        assert rec(0, p, p, pi, 1 << 29, 4, pi, pi, mat, 0, p, None, None) < 0 and b"2^29" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1 << 29, p, mat, 0, p, None, p, p, None) < 0 and b"2^29" in lib.hfem_last_error()
        bad = (C.c_double * 4)(1.0, 2.0, 1.0, 0.35)                                                    # c11 c22 - c12^2 < 0
        assert rec(0, p, p, pi, 1, 4, pi, pi, bad, 0, p, None, None) < 0 and b"positive definite" in lib.hfem_last_error()
    assert lib.hfem_quad4_von_mises(-7, None, None, None, 0, 1e9, 0.3, None, None, None) == 0
    assert lib.hfem_quad4_von_mises(0, p, p, pi, 1, 1e9, 0.3, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
    assert lib.hfem_quad4_von_mises(0, p, p, pi, -1, 1e9, 0.3, p, None, None) < 0 and b"negative" in lib.hfem_last_error()


def test_stress_recovery_refuses_a_cpu_model():
    """No CPU fallback: the object says so instead of failing inside a launch."""
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    from hidenn_fem_amd.post import StressRecovery
    coords, conn = Z.meshes()["tri_structured"][:2]
    m = PiecewiseLinearShapeNN2D(coords, conn)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StressRecovery(m, EnergyLoss2D(device=torch.device("cpu"), dtype=F64))
