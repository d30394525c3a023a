"""The CPU statement of the QUAD4 Neo-Hookean total potential (tests/quad4_hyper_reference.py) pinned on its own, on the meshes
and the finite-strain field the device tests use (tests/test_gpu_quad4_neo_hookean.py), and the element's source text
(csrc/hfem_quad4_hyper_dev.h) compiled as host C++ under the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import quad4_hyper_reference as Q

F64 = torch.float64
MESHES = ["jittered", "split", "mixed"]
_cache = {}


def mesh(name):
    if "meshes" not in _cache:
        _cache["meshes"] = Q.meshes()
    return _cache["meshes"][name]


def setup(name):
    coords, conn = mesh(name)[:2]
    lam, mu = Q.lame()
    return coords, conn, lam, mu


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def b_force(x):
    return torch.stack([2e9 * (1 + x[:, 0]), -1e9 * x[:, 1]], dim=1)


def test_meshes_are_what_the_tests_say():
    """17 x 9 jittered nodes; the split Delaunay mesh of 150 points (valence 1..9: far from the structured grid's 4); its
    renumbering with half the cells clockwise."""
    import quad_meshes as QM
    assert mesh("jittered")[1].shape == (128, 4) and mesh("plate")[5].shape[0] > 0
    coords, conn = mesh("split")[:2]
    val = QM.valence(conn.numpy(), coords.shape[0])
    assert val.min() == 1 and val.max() == 9
    X = mesh("mixed")[0][mesh("mixed")[1]]
    d1, d2 = X[:, 2] - X[:, 0], X[:, 3] - X[:, 1]
    cw = int(((d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]) < 0).sum())
    assert cw == conn.shape[0] // 2


@pytest.mark.parametrize("name", MESHES)
def test_closed_form_gradients_equal_autograd_through_the_textbook_formula(name):
    """Energy and both gradients against autograd through mu/2 (tr F^T F - 2) - mu ln J + lambda/2 ln^2 J at the four points,
    on the finite-strain field: 1e-13 max|g|; the energy 1e-13 relative."""
    coords, conn, lam, mu = setup(name)
    u = Q.field(coords)
    r = Q.total(coords, u, conn, lam, mu)
    loss, gx, gu = Q.naive_total(coords, u, conn, lam, mu)
    print(name, abs(r["loss"] - loss) / abs(loss), rel(r["gX"], gx), rel(r["gU"], gu))
    assert abs(r["loss"] - loss) <= 1e-13 * abs(loss)
    assert rel(r["gX"], gx) <= 1e-13 and rel(r["gU"], gu) <= 1e-13


@pytest.mark.parametrize("name", MESHES)
def test_homogeneous_patch(name):
    """u = (F0 - I) x: Pi = area psi(F0) within 1e-13 relative (the 2x2 rule integrates the linear det J exactly), interior
    rows of both gradients <= 1e-12 max|g|, J = det F0 at every point."""
    coords, conn, lam, mu = setup(name)
    geom = mesh(name)[2]
    r = Q.total(coords, Q.patch_field(coords), conn, lam, mu)
    want = Q.area(coords, conn) * Q.psi_of_F(Q.F0, lam, mu).item()
    assert abs(r["loss"] - want) <= 1e-13 * abs(want)
    interior = ~geom
    assert interior.sum() > 10
    for g in (r["gX"], r["gU"]):
        assert g[interior].abs().max() <= 1e-12 * g.abs().max()
    assert abs(r["min_J"] - torch.linalg.det(Q.F0).item()) <= 1e-13 and r["count"] == 0
    t = Q.element_terms(coords, Q.patch_field(coords), conn, lam, mu)
    assert (t["J"] - torch.linalg.det(Q.F0)).abs().max() <= 1e-13


@pytest.mark.parametrize("name", MESHES)
def test_objectivity(name):
    """u -> R (x + u) - x, R a rotation by 0.7 rad, leaves Pi unchanged within 1e-13 relative."""
    coords, conn, lam, mu = setup(name)
    u = Q.field(coords)
    a = Q.total(coords, u, conn, lam, mu)["loss"]
    b = Q.total(coords, Q.rotate_field(coords, u), conn, lam, mu)["loss"]
    assert abs(a - b) <= 1e-13 * abs(a)


@pytest.mark.parametrize("name", MESHES)
def test_small_strain_limit_is_the_linear_physical_energy(name):
    """Pi(eps u) / eps^2 and the gradients against oracle.quad4.quad4_domain_energy(convention="physical"): the deviation is
    first order in eps (ratio 9-11 between 1e-3 and 1e-4) and still shrinking at 1e-6 -- no cancellation.  The three
    first-order constants (deviation / eps at 1e-4; energy, d/dx, d/du) are printed; DESIGN 19 records them."""
    coords, conn, lam, mu = setup(name)
    u = Q.field(coords)
    lin, lgx, lgu = Q.linear_physical(coords, u, conn)
    dev = {}
    for eps in (1e-3, 1e-4, 1e-5, 1e-6):
        r = Q.total(coords, eps * u, conn, lam, mu)
        dev[eps] = (abs(r["loss"] / eps ** 2 - lin) / abs(lin), rel(r["gX"] / eps ** 2, lgx), rel(r["gU"] / eps, lgu))
    print(name, {k: tuple(f"{x:.3e}" for x in v) for k, v in dev.items()})
    print(name, "constants", tuple(f"{x / 1e-4:.3f}" for x in dev[1e-4]))
    for q in range(3):
        assert 9.0 <= dev[1e-3][q] / dev[1e-4][q] <= 11.0, (q, dev)
        assert dev[1e-6][q] < dev[1e-5][q] < dev[1e-4][q], (q, dev)
        assert dev[1e-4][q] <= 1.0 * 1e-4                          # O(1) coefficient at max|H| ~ 0.5: well under 1 eps


@pytest.mark.parametrize("name", MESHES + ["plate"])
def test_finite_strain_field_stays_off_the_inversion_branch(name):
    """min J > 0.2 over all Gauss points (jitter 0.3, seed 4 on the structured mesh), so the parity tests never touch the
    inversion branch."""
    coords, conn, lam, mu = setup(name)
    r = Q.total(coords, Q.field(coords), conn, lam, mu)
    assert r["min_J"] > 0.2 and r["count"] == 0 and math.isfinite(r["loss"])


@pytest.mark.parametrize("name", MESHES)
def test_inversion_rule(name):
    """One interior node pushed across a cell's diagonal: exactly one cell inverted, loss +inf, that cell's sixteen entries
    zero, gradients finite and equal to the sum over the OTHER cells."""
    coords, conn, lam, mu = setup(name)
    v, n = Q.invert_one_cell(coords, Q.field(coords), conn)
    r = Q.total(coords, v, conn, lam, mu)
    assert r["count"] == 1 and r["loss"] == float("inf") and r["min_J"] < 0
    assert torch.isfinite(r["gX"]).all() and torch.isfinite(r["gU"]).all()
    t = Q.element_terms(coords, v, conn, lam, mu)
    bad = t["inverted"]
    assert int(bad.sum()) == 1 and (t["gX"][bad] == 0).all() and (t["gU"][bad] == 0).all() and t["e"][bad].item() == float("inf")
    assert torch.isfinite(t["e"][~bad]).all() and t["gU"][~bad].abs().max() > 0
    rest = Q.total(coords, v, conn[~bad], lam, mu)
    assert torch.equal(rest["gX"], r["gX"]) and torch.equal(rest["gU"], r["gU"]) and math.isfinite(rest["loss"])


def test_edge_and_body_terms_equal_autograd():
    """Dead loads: the edge work and the body force's share of the energy and both gradients against autograd."""
    coords, conn, lam, mu = setup("plate")
    edges = mesh("plate")[5]
    u = Q.field(coords)
    Bq = Q.body_points(b_force)
    T = Q.traction_table(coords, edges, lambda x: torch.stack([1e9 * (1 + x[:, 1]), 2e8 * x[:, 0]], dim=1))
    r = Q.total(coords, u, conn, lam, mu, Bq, edges, T)
    base = Q.total(coords, u, conn, lam, mu)
    x, w = coords.clone().requires_grad_(True), u.clone().requires_grad_(True)
    det = torch.linalg.det(torch.einsum("eki,qjk->eqij", x[conn], Q.DN))
    uh = torch.einsum("qk,eki->eqi", Q.N, w[conn])
    ds = (x[edges[:, 1]] - x[edges[:, 0]]).norm(dim=1)
    extra = -(det.abs() * (uh * Bq[None]).sum(-1)).sum() \
        - (ds * ((w[edges[:, 0]] * T[:, 0:2]).sum(1) + (w[edges[:, 1]] * T[:, 2:4]).sum(1))).sum()
    extra.backward()
    assert abs(r["loss"] - base["loss"] - extra.item()) <= 1e-13 * abs(r["loss"])
    assert rel(r["gX"] - base["gX"], x.grad) <= 1e-13 and rel(r["gU"] - base["gU"], w.grad) <= 1e-13


def test_element_source_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hfem_quad4_hyper_dev.h (the element; the finishing reduction's per-thread part comes with hfem_hyper_dev.h) as plain
    C++ against a stub <hip/hip_runtime.h>, built with -fsanitize=address,undefined as a stand-alone program and run as a child
    process, on the mixed-orientation split mesh and the jittered mesh, plain, with one inverted cell and with a body table:
    every cell's energy, four J values and sixteen gradient entries, and the totals through the emulated reduction tree, within
    1e-12 of this module's numbers.  CPU only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "quad4_hyper_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "quad4_hyper_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    Bq = Q.body_points(b_force)
    counts = []
    for name in ("mixed", "jittered"):
        coords, conn, lam, mu = setup(name)
        inv_u = Q.invert_one_cell(coords, Q.field(coords), conn)[0]
        for tag, u, body in (("plain", Q.field(coords), None), ("body", Q.field(coords), Bq), ("inverted", inv_u, None),
                             ("inverted_body", inv_u, Bq)):
            t = Q.element_terms(coords, u, conn, lam, mu, body)
            tot = Q.total(coords, u, conn, lam, mu, body)
            path = str(tmp_path / f"{name}_{tag}.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<3q", conn.shape[0], coords.shape[0], 37))
                f.write(struct.pack("<10d", lam, mu, *(body.reshape(-1).tolist() if body is not None else [0.0] * 8)))
                f.write(conn.numpy().astype(np.int32).tobytes())
                for a in (coords, u, t["e"], t["J"], t["gX"], t["gU"]):
                    f.write(np.ascontiguousarray(a.numpy(), dtype=np.float64).tobytes())
                f.write(struct.pack("<3d", tot["loss"], tot["min_J"], float(tot["count"])))
            run = subprocess.run([exe, path], capture_output=True, text=True)
            print(name, tag, run.stdout.strip())
            assert run.returncode == 0, run.stdout + run.stderr
            counts.append(tot["count"])
    assert counts == [0, 0, 1, 1] * 2
