"""The CPU statement of the Cauchy stress recovery and the finite-strain ZZ indicator (tests/hyper_zz_reference.py) pinned by
what it must satisfy on its own -- closed form against autograd, patch test, objectivity, numbering, quadrature, the
small-strain limit, the inversion rule, the refinement rate --, the per-point source text (csrc/hfem_recover_hyper_dev.h)
compiled as host C++ under the address and undefined-behaviour sanitizers, and the host side of the feature: the four new
symbols' argument checks and the refusals of ``HyperStressRecovery``.  No GPU."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import hyper_reference as H
import hyper_zz_reference as HZ
import zz_reference as Z
from oracle import ref_chain as R

F64 = torch.float64
LAM, MU = H.lame()


@pytest.fixture(scope="module")
def meshes():
    return HZ.meshes()


@pytest.fixture(scope="module")
def results(meshes):
    """name -> the statement on the finite-strain field: computed once, shared, never modified."""
    return {k: HZ.zz(m[0], HZ.field(m[0]), m[1], LAM, MU) for k, m in meshes.items()}


def rotate_voigt(sig, angle):
    c, s = math.cos(angle), math.sin(angle)
    Q = torch.tensor([[c, -s], [s, c]], dtype=F64)
    T = torch.stack([torch.stack([sig[:, 0], sig[:, 2]], 1), torch.stack([sig[:, 2], sig[:, 1]], 1)], 1)
    T = Q @ T @ Q.T
    return torch.stack([T[:, 0, 0], T[:, 1, 1], T[:, 0, 1]], 1)


def test_the_field_inverts_nothing_on_the_five_meshes(meshes, results):
    sizes = {k: (m[0].shape[0], m[1].shape[0]) for k, m in meshes.items()}
    assert sizes == {"tri_structured": (391, 704), "tri_unstructured": (364, 615), "quad_structured": (437, 396),
                     "quad_split": (752, 681), "quad_split_renumbered": (752, 681)}
    for name, r in results.items():
        assert r["inverted"] == 0 and 0.309 <= r["J"].min().item() and r["J"].max().item() <= 2.04, name
        assert r["min_J"] == r["J"].min().item()


def test_linearisation_at_the_identity_is_the_plane_stress_C():
    """``plane="stress"``: C0 is EnergyLoss2D's C entry for entry."""
    assert (HZ.C0(LAM, MU) - R.plane_stress_C()).abs().max().item() <= 1e-15 * R.plane_stress_C().max().item()


def test_autograd_stress_equals_the_closed_form(meshes, results):
    for name, (coords, conn, *_) in meshes.items():
        F, _ = HZ.deformation_gradients(coords, HZ.field(coords), conn)
        closed = HZ.cauchy_closed(F, LAM, MU)
        err = (results[name]["sig_h"] - closed).abs().max().item() / closed.abs().max().item()
        print(f"{name}: autograd vs closed form {err:.2e}")
        assert err <= 1e-12, name


def test_patch_field_homogeneous_deformation(meshes):
    F0 = H.F0
    P = MU * (F0 - torch.linalg.inv(F0).T) + LAM * math.log(torch.linalg.det(F0).item()) * torch.linalg.inv(F0).T
    s = P @ F0.T / torch.linalg.det(F0)
    const = torch.tensor([s[0, 0], s[1, 1], s[0, 1]], dtype=F64)
    for name, (coords, conn, *_) in meshes.items():
        r = HZ.zz(coords, HZ.patch_field(coords), conn, LAM, MU)
        print(f"{name}: eta_rel {r['relative']:.3e}")
        assert r["relative"] <= 1e-13, (name, r["relative"])
        used = torch.zeros(coords.shape[0], dtype=torch.bool)
        used[conn.reshape(-1)] = True
        assert (r["nodal_stress"][used] - const).abs().max().item() <= 1e-13 * const.abs().max().item(), name
        assert (r["nodal_J"][used] - torch.linalg.det(F0)).abs().max().item() <= 1e-13


def test_objectivity_under_a_superposed_rotation(meshes, results):
    for name, (coords, conn, *_) in meshes.items():
        a = results[name]
        b = HZ.zz(coords, HZ.rotate_field(coords, HZ.field(coords), 0.7), conn, LAM, MU)
        assert (a["eta2"] - b["eta2"]).abs().max().item() <= 1e-12 * a["eta2"].max().item(), name
        assert abs(a["eta2_total"] - b["eta2_total"]) <= 1e-12 * a["eta2_total"]
        assert abs(a["norm2_total"] - b["norm2_total"]) <= 1e-12 * a["norm2_total"]
        turned = rotate_voigt(a["nodal_stress"], 0.7)
        assert (turned - b["nodal_stress"]).abs().max().item() <= 1e-12 * turned.abs().max().item(), name
        assert (a["nodal_J"] - b["nodal_J"]).abs().max().item() <= 1e-12


def test_renumbering_leaves_the_totals_unchanged(results):
    a, b = results["quad_split"], results["quad_split_renumbered"]
    assert abs(a["eta2_total"] - b["eta2_total"]) <= 1e-13 * a["eta2_total"]
    assert abs(a["norm2_total"] - b["norm2_total"]) <= 1e-13 * a["norm2_total"]


def test_tri3_closed_form_equals_three_point_quadrature(meshes, results):
    for name in ("tri_structured", "tri_unstructured"):
        coords, conn = meshes[name][:2]
        b = HZ.zz(coords, HZ.field(coords), conn, LAM, MU, tri_rule="quad3")["eta2"]
        assert (results[name]["eta2"] - b).abs().max().item() <= 1e-13 * b.max().item(), name


def test_small_strain_limit_is_the_linear_zz_estimate(meshes):
    """u = a zz_reference.field / 1e-4: eta_e^2 / a^2 deviates from the linear estimate (physical convention) at first order
    in the strain, so the deviation falls >= 5x from a = 1e-3 to 1e-4 (first order: 10x; a factor 2 for second-order terms)."""
    C = R.plane_stress_C()
    for name, (coords, conn, *_) in meshes.items():
        dev = {}
        for a in (1e-3, 1e-4):
            u = a * Z.field(coords) / 1e-4
            h = HZ.zz(coords, u, conn, LAM, MU)
            lin = Z.zz(coords, u, conn, C, "physical")
            dev[a] = ((h["eta2"] - lin["eta2"]).abs().max() / lin["eta2"].max()).item()       # the common 1 / a^2 cancels
        print(f"{name}: deviation {dev[1e-3]:.3e} -> {dev[1e-4]:.3e} ({dev[1e-3] / dev[1e-4]:.2f}x)")
        assert dev[1e-4] > 0.0 and dev[1e-3] / dev[1e-4] >= 5.0, (name, dev)


@pytest.mark.parametrize("name", ["tri_structured", "quad_split"])
def test_inversion_rule(meshes, name):
    coords, conn = meshes[name][:2]
    u0 = HZ.field(coords)
    u, node = (HZ.invert_one_element if conn.shape[1] == 3 else HZ.invert_one_cell)(coords, u0, conn)
    r, base = HZ.zz(coords, u, conn, LAM, MU), HZ.zz(coords, u0, conn, LAM, MU)
    assert r["inverted"] == 1 and int(torch.isinf(r["eta2"]).sum()) == 1 and r["min_J"] <= 0.0
    assert torch.isinf(r["eta2"][r["inverted_mask"]]).all() and r["norm2"][r["inverted_mask"]].item() == 0.0
    for k in ("nodal_stress", "nodal_J", "area", "eta2", "norm2", "sig_h", "J"):
        assert not torch.isnan(r[k]).any(), k
    assert r["relative"] == 1.0 and math.isinf(r["eta"]) and math.isfinite(r["norm2_total"])
    # the inverted element has left the projection: its nodes lost its share of the lumped area, nothing else did
    e = int(r["inverted_mask"].nonzero()[0])
    touched = torch.zeros(coords.shape[0], dtype=torch.bool)
    touched[conn[e]] = True
    assert (r["area"][touched] < base["area"][touched]).all() and torch.equal(r["area"][~touched], base["area"][~touched])


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_eta_halves_per_refinement(kind):
    """eta(n) / eta(2n - 1) on the structured n x n meshes of [0, 2] x [0, 1] with the finite-strain field, measured with
    this statement on the CPU: TRI3 2.0844, 2.0628, 2.0233 and QUAD4 2.1316, 2.0821, 2.0281 at n = 9, 17, 33 -- approaching 2
    (eta = O(h) with a superconvergent recovery).  Asserted within +-5 % of those values."""
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    mesher = structured_tri_mesh if kind == "tri" else structured_quad_mesh
    measured = {"tri": (2.0844, 2.0628, 2.0233), "quad": (2.1316, 2.0821, 2.0281)}[kind]
    cache = {}

    def eta(n):
        if n not in cache:
            coords, conn = mesher(n, n, dtype=F64)[:2]
            cache[n] = HZ.zz(coords, HZ.field(coords), conn, LAM, MU)["eta"]
        return cache[n]

    for n, want in zip((9, 17, 33), measured):
        ratio = eta(n) / eta(2 * n - 1)
        print(f"{kind} n {n}: eta(n)/eta(2n-1) = {ratio:.4f}")
        assert 0.95 * want <= ratio <= 1.05 * want, (kind, n, ratio)


# ---------------------------------------------------------------- the per-point source text under the sanitizers
def test_point_and_indicator_source_under_address_and_ub_sanitizers(tmp_path, meshes):
    """csrc/hfem_recover_hyper_dev.h (the Cauchy law, the element's points and the element's indicator: the text the kernels
    compile) as plain C++ against a stub <hip/hip_runtime.h>, built with -fsanitize=address,undefined, on the jittered TRI3
    mesh and the QUAD4 split mesh, each with and without an inverted element: every point's sigma and j and every element's
    eta_e^2 within 1e-12 of this module's numbers.  CPU only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "hyper_recover_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "hyper_recover_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    counts = []
    for name in ("tri_structured", "quad_split"):
        coords, conn = meshes[name][:2]
        u0 = HZ.field(coords)
        inv = (HZ.invert_one_element if conn.shape[1] == 3 else HZ.invert_one_cell)(coords, u0, conn)[0]
        for tag, u in (("plain", u0), ("inverted", inv)):
            t = HZ.zz(coords, u, conn, LAM, MU)
            sig = t["sig_h"].clone()
            sig[t["inverted_mask"]] = float("nan")                   # masked everywhere: not compared
            path = str(tmp_path / f"{name}_{tag}.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<3q", conn.shape[0], coords.shape[0], conn.shape[1]))
                f.write(struct.pack("<2d", LAM, MU))
                f.write(conn.numpy().astype(np.int32).tobytes())
                for a in (coords, u, t["nodal_stress"], sig, t["J"] - 1.0, t["eta2"]):
                    f.write(np.ascontiguousarray(a.numpy(), dtype=np.float64).tobytes())
            run = subprocess.run([exe, path], capture_output=True, text=True)
            print(name, tag, run.stdout.strip())
            assert run.returncode == 0, run.stdout + run.stderr
            counts.append(t["inverted"])
    assert counts == [0, 1, 0, 1]


# ---------------------------------------------------------------- the C ABI's argument checks (no device is touched)
NEW_SYMBOLS = ["hfem_tri3_hyper_stress_recover", "hfem_quad4_hyper_stress_recover", "hfem_tri3_hyper_zz_error",
               "hfem_quad4_hyper_zz_error"]


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
    for kind in ("hyper_stress_recover", "hyper_zz_error"):
        assert L.PROTOTYPES[f"hfem_quad4_{kind}"] == L.PROTOTYPES[f"hfem_tri3_{kind}"]
    lib = L.lib()
    assert lib.hfem_version() == 114                                  # append-only: the version stays
    buf = (C.c_double * 16)()
    ibuf = (C.c_int32 * 16)()
    p, pi = C.addressof(buf), C.addressof(ibuf)            # never dereferenced: every call below returns before a launch
    lame = (C.c_double * 2)(LAM, MU)
    for kind in ("tri3", "quad4"):
        rec, zz = getattr(lib, f"hfem_{kind}_hyper_stress_recover"), getattr(lib, f"hfem_{kind}_hyper_zz_error")
        assert rec(-7, None, None, None, 0, 5, None, None, None, None, None, None, None) == 0     # not even the device id is read
        assert rec(-7, None, None, None, 5, 0, None, None, None, None, None, None, None) == 0
        assert zz(-7, None, None, None, 0, None, None, None, None, None, None, None) == 0
        assert rec(0, p, p, pi, 1, 4, pi, pi, lame, None, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert rec(0, p, p, pi, 1, 4, pi, pi, None, p, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, lame, None, None, p, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, lame, p, None, p, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1, p, lame, p, None, None, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert rec(0, p, p, pi, -1, 4, pi, pi, lame, p, None, None, None) < 0 and b"negative" in lib.hfem_last_error()
        assert rec(0, p, p, pi, 1, -4, pi, pi, lame, p, None, None, None) < 0 and b"negative" in lib.hfem_last_error()
        assert zz(0, p, p, pi, -1, p, lame, p, None, p, p, None) < 0 and b"negative" in lib.hfem_last_error()
        assert rec(0, p, p, pi, 1 << 29, 4, pi, pi, lame, p, None, None, None) < 0 and b"2^29" in lib.hfem_last_error()
        assert zz(0, p, p, pi, 1 << 29, p, lame, p, None, p, p, None) < 0 and b"2^29" in lib.hfem_last_error()
        for bad in ((1.0, 0.0), (1.0, -1.0), (-2.0, 1.0), (float("nan"), 1.0)):                  # mu > 0 and lambda + mu > 0
            bl = (C.c_double * 2)(*bad)
            assert rec(0, p, p, pi, 1, 4, pi, pi, bl, p, None, None, None) < 0 and b"positive definite" in lib.hfem_last_error()
            assert zz(0, p, p, pi, 1, p, bl, p, None, p, p, None) < 0 and b"positive definite" in lib.hfem_last_error()


# ---------------------------------------------------------------- refusals (CPU models: nothing is launched)
def cpu_model(kind):
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    coords, conn = HZ.meshes()["tri_structured" if kind == "tri" else "quad_structured"][:2]
    return PiecewiseLinearShapeNN2D(coords, conn)


def test_hyper_stress_recovery_refuses_a_cpu_model():
    from hidenn_fem_amd.loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    from hidenn_fem_amd.post import HyperStressRecovery, hyper_zz_error, recover_cauchy_stress
    cpu = torch.device("cpu")
    for kind, cls in (("tri", NeoHookeanLoss2D), ("quad", Quad4NeoHookeanLoss2D)):
        m, loss_fn = cpu_model(kind), cls(device=cpu, dtype=F64)
        for make in (HyperStressRecovery, hyper_zz_error, recover_cauchy_stress):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                make(m, loss_fn)


def test_hyper_stress_recovery_refuses_the_wrong_loss_kinds():
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    from hidenn_fem_amd.post import HyperStressRecovery, StressRecovery
    cpu = torch.device("cpu")
    tri, quad = cpu_model("tri"), cpu_model("quad")
    for m in (tri, quad):
        with pytest.raises(NotImplementedError, match="StressRecovery"):
            HyperStressRecovery(m, EnergyLoss2D(device=cpu, dtype=F64))
        with pytest.raises(NotImplementedError):
            HyperStressRecovery(m, object())
    with pytest.raises(NotImplementedError, match="TRI3"):
        HyperStressRecovery(quad, NeoHookeanLoss2D(device=cpu, dtype=F64))
    with pytest.raises(NotImplementedError, match="QUAD4"):
        HyperStressRecovery(tri, Quad4NeoHookeanLoss2D(device=cpu, dtype=F64))
    # the linear class keeps refusing finite-strain losses, and says where to go
    for m, cls in ((tri, NeoHookeanLoss2D), (quad, Quad4NeoHookeanLoss2D)):
        with pytest.raises(NotImplementedError, match="HyperStressRecovery"):
            StressRecovery(m, cls(device=cpu, dtype=F64))
