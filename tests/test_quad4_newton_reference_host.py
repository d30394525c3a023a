"""The CPU statement of the QUAD4 Neo-Hookean tangent and of the inexact Newton solve on it (tests/quad4_newton_reference.py)
pinned on its own, on the meshes and the finite-strain field the device tests use (tests/test_gpu_quad4_newton.py), and the
element tangent's source text (csrc/hfem_quad4_hyper_dev.h) compiled as host C++ under the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import newton_reference as N
import quad4_hyper_reference as Q
import quad4_newton_reference as QN

F64 = torch.float64
MESHES = ["jittered", "split", "mixed", "plate"]
_cache = {}


def mesh(name):
    if "meshes" not in _cache:
        _cache["meshes"] = Q.meshes()
    return _cache["meshes"][name]


def tangent_at_field(name, scale=1.0):
    if ("K", name, scale) not in _cache:
        coords, conn = mesh(name)[:2]
        lam, mu = Q.lame()
        _cache[("K", name, scale)] = QN.dense_tangent(coords, scale * Q.field(coords), conn, lam, mu)
    return _cache[("K", name, scale)]


@pytest.mark.parametrize("name", MESHES)
def test_tangent_equals_the_autograd_hessian_of_the_energy(name):
    """K_T by the closed form against torch.autograd.functional.hessian of ``Q.element_terms``' energy at ``Q.field``:
    1e-13 max|K| (measured <= 4e-16); K_T is symmetric to the same bound."""
    coords, conn = mesh(name)[:2]
    lam, mu = Q.lame()
    K = tangent_at_field(name)
    hess = torch.autograd.functional.hessian(
        lambda v: Q.element_terms(coords, v.reshape(-1, 2), conn, lam, mu)["e"].sum(), Q.field(coords).reshape(-1).clone())
    err, sym = ((K - hess).abs().max() / K.abs().max()).item(), ((K - K.T).abs().max() / K.abs().max()).item()
    print(name, "hessian", err, "symmetry", sym)
    assert err <= 1e-13 and sym <= 1e-13


@pytest.mark.parametrize("name,negative", [("jittered", 4), ("split", 11), ("mixed", 11), ("plate", 4)])
def test_tangent_is_indefinite_at_the_test_field(name, negative):
    """What makes the device apply test cover the indefinite case: 4, 11, 11 and 4 negative eigenvalues."""
    ev = torch.linalg.eigvalsh(tangent_at_field(name))
    n = int((ev < -1e-9 * ev.abs().max()).sum())
    print(name, "negative eigenvalues", n, "smallest", ev[0].item(), "largest", ev[-1].item())
    assert n == negative


@pytest.mark.parametrize("name", MESHES)
def test_diagonal_blocks_are_positive_definite_up_to_1_75_and_not_at_2(name):
    """The device test of the identity fallback scales the field in steps of 0.25 until a block is not positive definite:
    none at 1.0 .. 1.75 x the field, some at 2.0 (with a few inverted cells, which contribute zero)."""
    coords, conn = mesh(name)[:2]
    lam, mu = Q.lame()
    for scale in (1.0, 1.25, 1.5, 1.75):
        assert N.jacobi_inverse(N.diag_blocks(tangent_at_field(name, scale)))[1].all()
    bad = int((~N.jacobi_inverse(N.diag_blocks(tangent_at_field(name, 2.0)))[1]).sum())
    inv = Q.total(coords, 2.0 * Q.field(coords), conn, lam, mu)["count"]
    print(name, "blocks not positive definite at 2.0:", bad, "inverted cells", inv)
    assert bad > 0 and inv > 0


@pytest.mark.parametrize("name", MESHES)
def test_closed_form_corner_blocks_equal_the_unit_direction_blocks(name):
    """K_aa = sum_q A [mu |w|^2 I + (mu - lambda L + lambda) t (x) t] against the blocks read off the 8 x 8 tangents:
    1e-13 (measured <= 4e-16)."""
    coords, conn = mesh(name)[:2]
    lam, mu = Q.lame()
    u = Q.field(coords)
    a, b = QN.corner_blocks(coords, u, conn, lam, mu), QN.unit_blocks(QN.element_tangent(coords, u, conn, lam, mu))
    err = ((a - b).abs().max() / b.abs().max()).item()
    print(name, "closed-form blocks", err)
    assert err <= 1e-13


@pytest.mark.parametrize("name", MESHES)
def test_small_strain_limit_is_the_linear_stiffness(name):
    """K_T at u = 0 equals the dense Hessian of the oracle's linear QUAD4 energy in the physical convention."""
    from oracle import quad4 as OQ, ref_chain as R
    coords, conn = mesh(name)[:2]
    lam, mu = Q.lame()
    K = QN.dense_tangent(coords, torch.zeros_like(coords), conn, lam, mu)
    C = R.plane_stress_C(10e9, 0.3).to(F64)
    lin = torch.autograd.functional.hessian(
        lambda v: OQ.quad4_domain_energy(coords, v.reshape(-1, 2), conn, C, None, convention="physical"),
        torch.zeros(coords.numel(), dtype=F64))
    err = ((K - lin).abs().max() / lin.abs().max()).item()
    print(name, "K_T(0) against the linear Hessian", err)
    assert err <= 1e-13


def test_inverted_cell_contributes_a_zero_block():
    coords, conn = mesh("plate")[:2]
    lam, mu = Q.lame()
    v, _ = Q.invert_one_cell(coords, Q.field(coords), conn)
    t = Q.element_terms(coords, v, conn, lam, mu)
    Ke = QN.element_tangent(coords, v, conn, lam, mu)
    assert int(t["inverted"].sum()) == 1
    assert Ke[t["inverted"]].abs().max() == 0 and Ke[~t["inverted"]].abs().amax(dim=(1, 2)).min() > 0
    assert QN.corner_blocks(coords, v, conn, lam, mu)[t["inverted"]].abs().max() == 0
    K = QN.dense_tangent(coords, v, conn, lam, mu)
    assert torch.equal(K, QN.dense_tangent(coords, v, conn[~t["inverted"]], lam, mu))
    assert torch.equal(K, QN.dense_tangent(coords, v, conn, lam, mu, skip=t["inverted"]))


def test_plate_tangent_is_positive_definite_at_0_05_of_the_field_and_not_at_0_3():
    """The graph test of tests/test_gpu_quad4_newton.py needs a positive definite operator: the plate's free rows (left edge
    clamped at the field's values) at 0.05 x the field; TRI3's 0.3 is indefinite here, and so is 0.1."""
    coords, conn, _, bc = mesh("plate")[:4]
    lam, mu = Q.lame()
    ev = {s: torch.linalg.eigvalsh(N.restrict(tangent_at_field("plate", s), ~bc))[0].item() for s in (0.05, 0.1, 0.3)}
    print("smallest eigenvalue over the free rows", ev)
    assert ev[0.05] > 0 and ev[0.1] < 0 and ev[0.3] < 0


@pytest.mark.parametrize("name", list(N.RUNS))
def test_reference_driver_converges_within_the_caps(name):
    """The QUAD4 plate, E = 2e6, left edge clamped.  Measured: default traction 5 Newton / 323 CG iterations, all steps 1;
    traction (0, -4e4) 8 / 474, steps 0.5, 1, 0.5, then 1; no loads from ``Q.field`` 8 / 317 after one truncation on negative
    curvature, in Newton iteration 0 (after 11 CG iterations: the direction reached is taken)."""
    prob, r, g_start = QN.reference_run(name)
    caps = N.RUNS[name][3]
    g0 = r.rhs_norm if N.RUNS[name][1] else g_start
    print(name, r.newton_iterations, r.cg_iterations, r.reason, r.grad_norm / g0, [h["step"] for h in r.history],
          [(h["cg_reason"], h["cg_iterations"]) for h in r.history],
          "lambda_min", torch.linalg.eigvalsh(prob.tangent(r.u))[0].item())
    assert r.converged and r.newton_iterations <= caps[0] and r.cg_iterations <= caps[1]
    assert r.grad_norm <= 1e-10 * g0
    assert all(h["min_J"] > 0 for h in r.history)
    if name == "default":
        assert all(h["step"] == 1.0 for h in r.history)
    if name == "down":
        assert [h["step"] for h in r.history][:4] == [0.5, 1.0, 0.5, 1.0] and all(h["step"] == 1.0 for h in r.history[4:])
    if name == "relax":
        assert [h["cg_reason"] for h in r.history].count("breakdown") == 1
        assert r.history[0]["cg_reason"] == "breakdown" and r.history[0]["cg_iterations"] > 0
        assert abs(r.energy) <= 1e-20 * abs(r.history[0]["energy"]) and r.u.abs().max() <= 1e-11


def test_element_tangent_source_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hfem_quad4_hyper_dev.h's tangent apply and corner blocks as plain C++ against the stub <hip/hip_runtime.h>, built
    with -fsanitize=address,undefined as a stand-alone program and run as a child process, on the mixed-orientation split mesh
    and the plate: every cell's K_e p_e, p_e . q_e, four J values and the twelve entries of its four corner blocks within 1e-12
    of this module's numbers, and the apply on the c_q = mu - lambda L_q the blocks return (what the apply kernel reads behind a
    diag launch) bit-equal to the apply that recomputes them; one case per mesh has an inverted cell (exactly zero output,
    counted once).  CPU only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "quad4_hyper_tangent_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "quad4_hyper_tangent_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    lam, mu = Q.lame()
    for name in ("mixed", "plate"):
        coords, conn = mesh(name)[:2]
        p = torch.rand(coords.shape, dtype=F64, generator=torch.Generator().manual_seed(3)) - 0.5
        for tag, u in (("plain", Q.field(coords)), ("inverted", Q.invert_one_cell(coords, Q.field(coords), conn)[0])):
            Ke = QN.element_tangent(coords, u, conn, lam, mu)
            t = Q.element_terms(coords, u, conn, lam, mu)
            pe = p[conn].reshape(-1, 8)
            q = torch.einsum("eij,ej->ei", Ke, pe)
            count = int(t["inverted"].sum())
            path = str(tmp_path / f"{name}_{tag}.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<2q", conn.shape[0], coords.shape[0]))
                f.write(struct.pack("<2d", lam, mu))
                f.write(conn.numpy().astype(np.int32).tobytes())
                for a in (coords, u, p, q, (pe * q).sum(1), t["J"], QN.unit_blocks(Ke)):
                    f.write(np.ascontiguousarray(a.numpy(), dtype=np.float64).tobytes())
                f.write(struct.pack("<d", float(count)))
            out = subprocess.run([exe, path], capture_output=True, text=True)
            print(name, tag, out.stdout.strip())
            assert out.returncode == 0, out.stdout + out.stderr
            assert count == (1 if tag == "inverted" else 0)
