"""The CPU statement of the Neo-Hookean tangent and of the inexact Newton solve on it (tests/newton_reference.py) pinned on
its own, on the meshes and the finite-strain field the device tests use (tests/test_gpu_newton.py), and the element tangent's
source text (csrc/hfem_hyper_dev.h) compiled as host C++ under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import hyper_reference as H
import newton_reference as N

F64 = torch.float64
MESHES = ["jittered", "delaunay", "plate"]
_cache = {}


def mesh(name):
    if "meshes" not in _cache:
        _cache["meshes"] = H.meshes()
    return _cache["meshes"][name]


def tangent_at_field(name):
    if ("K", name) not in _cache:
        coords, conn = mesh(name)[:2]
        lam, mu = H.lame()
        _cache[("K", name)] = N.dense_tangent(coords, H.field(coords), conn, lam, mu, H.tri_W())
    return _cache[("K", name)]


@pytest.mark.parametrize("name", MESHES)
def test_tangent_equals_the_autograd_hessian_of_the_energy(name):
    """K_T by the closed form against torch.autograd.functional.hessian of ``element_terms``' energy at ``H.field``:
    1e-13 max|K| (measured <= 6e-16); K_T is symmetric to the same bound."""
    coords, conn = mesh(name)[:2]
    lam, mu = H.lame()
    W = H.tri_W()
    K = tangent_at_field(name)
    hess = torch.autograd.functional.hessian(
        lambda v: H.element_terms(coords, v.reshape(-1, 2), conn, lam, mu, W)["e"].sum(), H.field(coords).reshape(-1).clone())
    err, sym = ((K - hess).abs().max() / K.abs().max()).item(), ((K - K.T).abs().max() / K.abs().max()).item()
    print(name, "hessian", err, "symmetry", sym)
    assert err <= 1e-13 and sym <= 1e-13


@pytest.mark.parametrize("name,negative", [("jittered", 4), ("delaunay", 6), ("plate", 4)])
def test_tangent_is_indefinite_at_the_test_field(name, negative):
    """What makes the device apply test cover the indefinite case: 4, 6 and 4 negative eigenvalues."""
    ev = torch.linalg.eigvalsh(tangent_at_field(name))
    n = int((ev < -1e-9 * ev.abs().max()).sum())
    print(name, "negative eigenvalues", n, "smallest", ev[0].item(), "largest", ev[-1].item())
    assert n == negative


@pytest.mark.parametrize("name", MESHES)
def test_small_strain_limit_is_the_linear_stiffness(name):
    """K_T at u = 0 equals the dense Hessian of the oracle's linear energy in the physical convention."""
    coords, conn = mesh(name)[:2]
    lam, mu = H.lame()
    K = N.dense_tangent(coords, torch.zeros_like(coords), conn, lam, mu, H.tri_W())
    from oracle import ref_chain as R
    xg, wg = R.triangle_gauss(4, F64)
    C = R.plane_stress_C(10e9, 0.3)
    lin = torch.autograd.functional.hessian(
        lambda v: R.domain_energy(coords, v.reshape(-1, 2), conn, C, xg, wg, None, "physical"), torch.zeros(coords.numel(), dtype=F64))
    err = ((K - lin).abs().max() / lin.abs().max()).item()
    print(name, "K_T(0) against the linear Hessian", err)
    assert err <= 1e-13


def test_inverted_element_contributes_a_zero_block():
    coords, conn = mesh("jittered")[:2]
    lam, mu = H.lame()
    v, _ = H.invert_one_element(coords, H.field(coords), conn)
    t = H.element_terms(coords, v, conn, lam, mu, H.tri_W())
    Ke = N.element_tangent(coords, v, conn, lam, mu, H.tri_W())
    assert int(t["inverted"].sum()) == 1
    assert Ke[t["inverted"]].abs().max() == 0 and Ke[~t["inverted"]].abs().amax(dim=(1, 2)).min() > 0
    K = N.dense_tangent(coords, v, conn, lam, mu, H.tri_W())
    assert torch.equal(K, N.dense_tangent(coords, v, conn[~t["inverted"]], lam, mu, H.tri_W()))


@pytest.mark.parametrize("name", list(N.RUNS))
def test_reference_driver_converges_within_the_caps(name):
    """The plate, E = 2e6, left edge clamped.  Measured: default traction 5 Newton / 338 CG iterations, all steps 1; traction
    (0, -4e4) 9 / 634, first step 0.25; no loads from ``H.field`` 10 / 518 after two truncations on negative curvature."""
    prob, r, g_start = N.reference_run(name)
    caps = N.RUNS[name][3]
    g0 = r.rhs_norm if N.RUNS[name][1] else g_start
    print(name, r.newton_iterations, r.cg_iterations, r.reason, r.grad_norm / g0, [h["step"] for h in r.history],
          [h["cg_reason"] for h in r.history])
    assert r.converged and r.newton_iterations <= caps[0] and r.cg_iterations <= caps[1]
    assert r.grad_norm <= 1e-10 * g0
    assert all(h["min_J"] > 0 for h in r.history)
    if name == "default":
        assert all(h["step"] == 1.0 for h in r.history)
    if name == "down":
        assert r.history[0]["step"] == 0.25
    if name == "relax":
        assert [h["cg_reason"] for h in r.history].count("breakdown") == 2
        assert abs(r.energy) <= 1e-20 * abs(r.history[0]["energy"]) and r.u.abs().max() <= 1e-12


def test_element_tangent_source_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hfem_hyper_dev.h's state + apply as plain C++ against the stub <hip/hip_runtime.h>, built with
    -fsanitize=address,undefined, on the jittered mesh: every element's K_e p_e, p_e . q_e, J and the nine entries of its three
    corner blocks within 1e-12 of this module's numbers; one case has an inverted element (zero output, counted)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "hyper_tangent_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "hyper_tangent_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    coords, conn = mesh("jittered")[:2]
    lam, mu = H.lame()
    W = H.tri_W()
    p = torch.rand(coords.shape, dtype=F64, generator=torch.Generator().manual_seed(3)) - 0.5
    count = None
    for tag, u in (("plain", H.field(coords)), ("inverted", H.invert_one_element(coords, H.field(coords), conn)[0])):
        Ke = N.element_tangent(coords, u, conn, lam, mu, W)
        t = H.element_terms(coords, u, conn, lam, mu, W)
        pe = p[conn].reshape(-1, 6)
        q = torch.einsum("eij,ej->ei", Ke, pe)
        blocks = torch.stack([torch.stack([Ke[:, 2 * a, 2 * a], 0.5 * (Ke[:, 2 * a, 2 * a + 1] + Ke[:, 2 * a + 1, 2 * a]),
                                           Ke[:, 2 * a + 1, 2 * a + 1]], dim=1) for a in range(3)], dim=1)
        count = int(t["inverted"].sum())
        path = str(tmp_path / f"{tag}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<2q", conn.shape[0], coords.shape[0]))
            f.write(struct.pack("<3d", lam, mu, W))
            f.write(conn.numpy().astype(np.int32).tobytes())
            for a in (coords, u, p, q, (pe * q).sum(1), t["J"], blocks):
                f.write(np.ascontiguousarray(a.numpy(), dtype=np.float64).tobytes())
            f.write(struct.pack("<d", float(count)))
        out = subprocess.run([exe, path], capture_output=True, text=True)
        print(out.stdout.strip())
        assert out.returncode == 0, out.stdout + out.stderr
        assert count == (1 if tag == "inverted" else 0)
