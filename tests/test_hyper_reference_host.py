"""The CPU statement of the Neo-Hookean total potential (tests/hyper_reference.py) pinned on its own, on the meshes and the
finite-strain field the device tests use (tests/test_gpu_neo_hookean.py), and the element's source text
(csrc/hfem_hyper_dev.h) compiled as host C++ under the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import hyper_reference as H

F64 = torch.float64
MESHES = ["jittered", "delaunay", "plate"]
_cache = {}


def mesh(name):
    if "meshes" not in _cache:
        _cache["meshes"] = H.meshes()
    return _cache["meshes"][name]


def setup(name):
    coords, conn = mesh(name)[:2]
    lam, mu = H.lame()
    return coords, conn, lam, mu, H.tri_W()


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("name", MESHES)
def test_closed_form_gradients_equal_autograd_through_the_textbook_formula(name):
    """(a) energy and both gradients against autograd through mu/2 (tr F^T F - 2) - mu ln J + lambda/2 ln^2 J on the
    finite-strain field: 1e-13 max|g|; the energy 1e-13 relative."""
    coords, conn, lam, mu, W = setup(name)
    u = H.field(coords)
    r = H.total(coords, u, conn, lam, mu, W)
    loss, gx, gu = H.naive_total(coords, u, conn, lam, mu, W)
    print(name, abs(r["loss"] - loss) / abs(loss), rel(r["gX"], gx), rel(r["gU"], gu))
    assert abs(r["loss"] - loss) <= 1e-13 * abs(loss)
    assert rel(r["gX"], gx) <= 1e-13 and rel(r["gU"], gu) <= 1e-13


def test_lame_constants_linearise_to_the_plane_stress_matrix():
    """c11 = c22 = lambda + 2 mu, c12 = lambda, c33 = mu is the linear loss's C entry for entry (plane="stress")."""
    from oracle import ref_chain as R
    lam, mu = H.lame(10e9, 0.3, "stress")
    C = R.plane_stress_C(10e9, 0.3)
    for got, want in ((lam + 2 * mu, C[0, 0]), (lam + 2 * mu, C[1, 1]), (lam, C[0, 1]), (mu, C[2, 2])):
        assert abs(got - want.item()) <= 1e-15 * abs(want.item())
    lam_e, mu_e = H.lame(10e9, 0.3, "strain")
    assert mu_e == mu and abs(lam_e - 10e9 * 0.3 / (1.3 * 0.4)) <= 1e-6


@pytest.mark.parametrize("name", MESHES)
def test_homogeneous_patch(name):
    """(b) u = (F0 - I) x: Pi = 2 W area psi(F0) within 1e-13 relative, interior rows of both gradients <= 1e-12 max|g|."""
    coords, conn, lam, mu, W = setup(name)
    geom = mesh(name)[2]
    r = H.total(coords, H.patch_field(coords), conn, lam, mu, W)
    X = coords[conn]
    area = 0.5 * ((X[:, 0, 0] - X[:, 2, 0]) * (X[:, 1, 1] - X[:, 2, 1]) - (X[:, 1, 0] - X[:, 2, 0]) * (X[:, 0, 1] - X[:, 2, 1])).abs().sum().item()
    want = 2 * W * area * H.psi_of_F(H.F0, lam, mu).item()
    assert abs(r["loss"] - want) <= 1e-13 * abs(want)
    interior = ~geom
    assert interior.sum() > 10
    for g in (r["gX"], r["gU"]):
        assert g[interior].abs().max() <= 1e-12 * g.abs().max()
    assert abs(r["min_J"] - torch.linalg.det(H.F0).item()) <= 1e-13 and r["count"] == 0


@pytest.mark.parametrize("name", MESHES)
def test_objectivity(name):
    """(c) u -> R (x + u) - x, R a rotation by 0.7 rad, leaves Pi unchanged within 1e-13 relative."""
    coords, conn, lam, mu, W = setup(name)
    u = H.field(coords)
    a = H.total(coords, u, conn, lam, mu, W)["loss"]
    b = H.total(coords, H.rotate_field(coords, u), conn, lam, mu, W)["loss"]
    assert abs(a - b) <= 1e-13 * abs(a)


@pytest.mark.parametrize("name", MESHES)
def test_small_strain_limit_is_the_linear_physical_energy(name):
    """(d) Pi(eps u) / eps^2 and the gradients against the oracle's linear energy in the physical convention: the deviation
    is first order in eps (ratio 9-11 between 1e-3 and 1e-4) and still shrinking at 1e-6 -- no cancellation."""
    coords, conn, lam, mu, W = setup(name)
    u = H.field(coords)
    lin, lgx, lgu = H.linear_physical(coords, u, conn)
    dev = {}
    for eps in (1e-3, 1e-4, 1e-5, 1e-6):
        r = H.total(coords, eps * u, conn, lam, mu, W)
        dev[eps] = (abs(r["loss"] / eps ** 2 - lin) / abs(lin), rel(r["gX"] / eps ** 2, lgx), rel(r["gU"] / eps, lgu))
    print(name, {k: tuple(f"{x:.3e}" for x in v) for k, v in dev.items()})
    for q in range(3):
        assert 9.0 <= dev[1e-3][q] / dev[1e-4][q] <= 11.0, (q, dev)
        assert dev[1e-6][q] < dev[1e-5][q] < dev[1e-4][q], (q, dev)
        assert dev[1e-4][q] <= 1.0 * 1e-4                          # O(1) coefficient at max|H| ~ 0.5: well under 1 eps


@pytest.mark.parametrize("name", MESHES)
def test_finite_strain_field_stays_off_the_inversion_branch(name):
    """(e) min J > 0.2 (by hand: >= 0.22), so the parity tests never touch the J <= 0 branch."""
    coords, conn, lam, mu, W = setup(name)
    r = H.total(coords, H.field(coords), conn, lam, mu, W)
    assert r["min_J"] > 0.2 and r["count"] == 0 and math.isfinite(r["loss"])


@pytest.mark.parametrize("name", MESHES)
def test_inversion_rule(name):
    """One interior node pushed across an opposite edge: exactly one element inverted, loss +inf, gradients finite and equal
    to the sum over the OTHER elements."""
    coords, conn, lam, mu, W = setup(name)
    v, n = H.invert_one_element(coords, H.field(coords), conn)
    r = H.total(coords, v, conn, lam, mu, W)
    assert r["count"] == 1 and r["loss"] == float("inf") and r["min_J"] < 0
    assert torch.isfinite(r["gX"]).all() and torch.isfinite(r["gU"]).all()
    t = H.element_terms(coords, v, conn, lam, mu, W)
    keep = ~t["inverted"]
    rest = H.total(coords, v, conn[keep], lam, mu, W)
    assert torch.equal(rest["gX"], r["gX"]) and torch.equal(rest["gU"], r["gU"]) and math.isfinite(rest["loss"])


def test_edge_and_body_terms_equal_autograd():
    """Dead loads: the edge work and the body table's share of both gradients against autograd."""
    coords, conn, lam, mu, W = setup("plate")
    edges = mesh("plate")[5]
    u = H.field(coords)
    Bk = H.body_table(lambda x: torch.stack([2e9 * (1 + x[:, 0]), -1e9 * x[:, 1]], dim=1))
    T = H.traction_table(coords, edges, lambda x: torch.stack([1e9 * (1 + x[:, 1]), 2e8 * x[:, 0]], dim=1))
    r = H.total(coords, u, conn, lam, mu, W, Bk, edges, T)
    base = H.total(coords, u, conn, lam, mu, W)
    x, w = coords.clone().requires_grad_(True), u.clone().requires_grad_(True)
    X, U, Jg, _ = H._parts(x, w, conn)
    ds = (x[edges[:, 1]] - x[edges[:, 0]]).norm(dim=1)
    extra = -(torch.linalg.det(Jg).abs() * (U * Bk[None]).sum(dim=(1, 2))).sum() \
        - (ds * ((w[edges[:, 0]] * T[:, 0:2]).sum(1) + (w[edges[:, 1]] * T[:, 2:4]).sum(1))).sum()
    extra.backward()
    assert abs(r["loss"] - base["loss"] - extra.item()) <= 1e-13 * abs(r["loss"])
    assert rel(r["gX"] - base["gX"], x.grad) <= 1e-13 and rel(r["gU"] - base["gU"], w.grad) <= 1e-13


def test_element_source_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hfem_hyper_dev.h (the element and the finishing reduction's per-thread part, the text the kernels compile) as
    plain C++ against a stub <hip/hip_runtime.h>, built with -fsanitize=address,undefined, on the jittered mesh with one
    inverted element and a body table: every element's energy, J and twelve gradient entries, and the totals through the
    emulated reduction tree, within 1e-12 of this module's numbers.  CPU only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "hyper_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "hyper_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    coords, conn, lam, mu, W = setup("jittered")
    Bk = H.body_table(lambda x: torch.stack([2e9 * (1 + x[:, 0]), -1e9 * x[:, 1]], dim=1))
    for tag, u in (("plain", H.field(coords)), ("inverted", H.invert_one_element(coords, H.field(coords), conn)[0])):
        t = H.element_terms(coords, u, conn, lam, mu, W, Bk)
        tot = H.total(coords, u, conn, lam, mu, W, Bk)
        path = str(tmp_path / f"{tag}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<3q", conn.shape[0], coords.shape[0], 37))
            f.write(struct.pack("<9d", lam, mu, W, *Bk.reshape(-1).tolist()))
            f.write(conn.numpy().astype(np.int32).tobytes())
            for a in (coords, u, t["e"], t["J"], t["gX"], t["gU"]):
                f.write(np.ascontiguousarray(a.numpy(), dtype=np.float64).tobytes())
            f.write(struct.pack("<3d", tot["loss"], tot["min_J"], float(tot["count"])))
        run = subprocess.run([exe, path], capture_output=True, text=True)
        print(run.stdout.strip())
        assert run.returncode == 0, run.stdout + run.stderr
    assert tot["count"] == 1
