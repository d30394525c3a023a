"""What the tangent AMG adds on the host, without a GPU: the u row codes of every corner in the AMG host setup
(``conn_u``, hfem_amg_host_copy level -1 which 4) beside the unchanged fan arrays, the sparse CPU statement of the assembled
tangent (tests/tangent_amg_reference.py) against the dense one, and the assembly kernel's row loop
(csrc/hfem_amg_hyper_dev.h) compiled as host C++ under the address and undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import hyper_reference as H
import newton_reference as N
import quad4_hyper_reference as Q
import quad4_newton_reference as QN
import tangent_amg_reference as TA
from test_amg_host import Host, _lib, _mesh, _row_maps
from test_solve_quad4_host import HostEx, _quad_mesh

F64 = torch.float64


def _case(kind):
    return _quad_mesh() if kind == "quad" else _mesh(kind)


# ---------------------------------------------------------------- 1. conn_u and the old codes
@pytest.mark.parametrize("kind", ["structured", "delaunay", "quad"])
@pytest.mark.parametrize("order_seed", [None, 5])
def test_conn_u_is_the_u_row_code_of_every_corner_and_the_fan_arrays_are_unchanged(kind, order_seed):
    conn, bc, xmask = _case(kind)
    u_src, x_src = _row_maps(~bc, order_seed), _row_maps(xmask, order_seed)
    host = HostEx(conn, x_src, u_src) if kind == "quad" else Host(conn, x_src, u_src)
    npe = conn.shape[1]
    cu = host.arr(-1, 4)
    assert cu.dtype == np.int32 and cu.shape == (conn.shape[0] * npe,)
    assert np.array_equal(cu.reshape(-1, npe), u_src[conn])
    assert (cu < 0).any() and (cu >= 0).any()
    fixed = np.sort(-1 - cu[cu < 0])
    assert fixed[0] == 0 and fixed[-1] == int(bc.sum()) - 1           # fixed row k is coded -1 - k
    # which 0..3 of level -1: the fan, recomputed (element ascending within a row)
    rows = u_src[conn]                                                  # [ne, npe]
    e_id, c_id = np.nonzero(rows >= 0)                                  # element-major, corner ascending
    order = np.argsort(rows[e_id, c_id], kind="stable")
    n_u = int((u_src >= 0).sum())
    fan_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[e_id, c_id], minlength=n_u))])
    assert np.array_equal(host.arr(-1, 0), fan_ptr)
    assert np.array_equal(host.arr(-1, 1), e_id[order]) and np.array_equal(host.arr(-1, 2), c_id[order])
    slots = host.arr(-1, 3).reshape(-1, npe)
    a_ptr, a_col = host.arr(0, 0), host.arr(0, 1)
    cols = rows[e_id[order]]                                            # the column every slot of a fan entry writes to
    assert np.array_equal(slots < 0, cols < 0)
    assert np.array_equal(a_col[slots[slots >= 0]], cols[cols >= 0])
    owner = np.repeat(np.arange(n_u), np.diff(fan_ptr))[:, None].repeat(npe, 1)[slots >= 0]
    assert np.all(a_ptr[owner] <= slots[slots >= 0]) and np.all(slots[slots >= 0] < a_ptr[owner + 1])
    top = host.info(-1)
    assert top[1] == n_u and top[2] == conn.shape[0] and top[3] == fan_ptr[-1] and top[5] == npe and top[6] == top[7] == 0
    n = host.arr(0, 0)
    assert len(n) == n_u + 1
    L = host.L
    import ctypes as C
    cnt = C.c_int64()
    assert L.hfem_amg_host_copy(host.h, -1, 5, None, C.byref(cnt)) < 0 and b"which" in L.hfem_last_error()
    assert L.hfem_amg_host_copy(host.h, 0, 11, None, C.byref(cnt)) < 0 and b"which" in L.hfem_last_error()


def test_the_new_entry_points_are_bound_and_report_null_arguments_as_codes():
    import ctypes as C
    L = _lib()
    for name in ("hfem_amg_assemble_hyper", "hfem_amg_setup_hyper"):
        assert name in L.PROTOTYPES and getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    lame = (C.c_double * 2)(1.0, 1.0)
    assert L.lib().hfem_amg_assemble_hyper(None, None, None, None, None, lame, 0.5, None) < 0
    assert b"null pointer" in L.lib().hfem_last_error()
    assert L.lib().hfem_amg_setup_hyper(None, None, None, None, None, lame, 0.5, None, None) < 0
    assert b"null pointer" in L.lib().hfem_last_error()
    assert L.lib().hfem_version() == 114


# ---------------------------------------------------------------- 2. the sparse statement
def _mesh17(kind, name):
    ms = H.meshes() if kind == "tri" else Q.meshes()
    return ms[name]


def _shuffled_rows(bc, seed):
    return _row_maps(~bc.numpy(), seed)


@pytest.mark.parametrize("kind,name", [("tri", "plate"), ("tri", "jittered"), ("quad", "plate"), ("quad", "jittered")])
@pytest.mark.parametrize("seed", [None, 7])
def test_sparse_reference_equals_the_dense_tangent_on_the_free_rows(kind, name, seed):
    """At ``field`` on the 17 x 9 meshes, Dirichlet rows from the mesh, node order and a shuffled row order: the same entries
    to summation order (1e-14 max|K|)."""
    coords, conn, _, bc = _mesh17(kind, name)[:4]
    u = H.field(coords)
    lam, mu = H.lame()
    if kind == "tri":
        dense = N.dense_tangent(coords, u, conn, lam, mu, H.tri_W())
    else:
        dense = QN.dense_tangent(coords, u, conn, lam, mu)
    u_src = np.asarray(_shuffled_rows(bc, seed), dtype=np.int64)
    K = TA.sparse_tangent(coords, u, conn, lam, mu, H.tri_W() if kind == "tri" else None, u_src).toarray()
    n = int((u_src >= 0).sum())
    assert K.shape == (2 * n, 2 * n)
    node_of = np.empty(n, dtype=np.int64)
    node_of[u_src[u_src >= 0]] = np.nonzero(u_src >= 0)[0]
    dof = (2 * node_of[:, None] + np.arange(2)[None, :]).reshape(-1)
    want = dense.numpy()[np.ix_(dof, dof)]
    err = np.abs(K - want).max() / np.abs(want).max()
    print(kind, name, seed, "sparse against dense", err)
    assert err <= 1e-14
    if seed is None:
        assert np.abs(want - N.restrict(dense, ~bc).numpy()).max() == 0.0


# ---------------------------------------------------------------- 3. the row loop under the sanitizers
def _build_san(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "amg_hyper_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "amg_hyper_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    return exe


def test_assembly_row_loop_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hfem_amg_hyper_dev.h's amg_hyper_row as plain C++ against the stub <hip/hip_runtime.h>, built with
    -fsanitize=address,undefined as a stand-alone program and run as a child process: the 17 x 9 TRI3 and QUAD4 plates
    (clamped left edge: Dirichlet columns dropped; fixed boundary coordinates: both row codes in use) at ``field`` with nonzero
    Dirichlet values and one inverted element / cell, shuffled rows, every buffer exactly the pattern's size.  The blocks equal
    the sparse statement's to 1e-12 max|K|."""
    exe = _build_san(tmp_path)
    from hidenn_fem_amd.models import ordered_row_maps
    for kind in ("tri", "quad"):
        coords, conn, geom, bc = _mesh17(kind, "plate")[:4]
        lam, mu = H.lame()
        W = H.tri_W() if kind == "tri" else 1.0
        if kind == "tri":
            u, _ = H.invert_one_element(coords, H.field(coords), conn)
            count = H.total(coords, u, conn, lam, mu, W)["count"]
        else:
            u, _ = Q.invert_one_cell(coords, H.field(coords), conn)
            count = Q.total(coords, u, conn, lam, mu)["count"]
        assert count == 1 and u[bc].abs().max() > 0
        rng = np.random.default_rng(3)
        ufree, xfree = ~bc.numpy(), ~geom.numpy()
        u_src = ordered_row_maps(ufree, rng.permutation(np.nonzero(ufree)[0]))
        x_src = ordered_row_maps(xfree, rng.permutation(np.nonzero(xfree)[0]))
        host = HostEx(conn.numpy(), x_src, u_src)
        npe = conn.shape[1]
        a_ptr, a_col = host.arr(0, 0), host.arr(0, 1)
        n_u = len(a_ptr) - 1
        K = TA.sparse_tangent(coords, u, conn, lam, mu, W if kind == "tri" else None, np.asarray(u_src, dtype=np.int64)).toarray()
        rows = np.repeat(np.arange(n_u), np.diff(a_ptr))
        want = np.stack([K[2 * r:2 * r + 2, 2 * c:2 * c + 2] for r, c in zip(rows, a_col)])
        assert np.count_nonzero(K) == np.count_nonzero(want)           # the pattern holds every entry

        def table(vals, src, free):
            out = np.zeros((int(free.sum()), 2)), np.zeros((int((~free).sum()), 2))
            s = np.asarray(src)
            out[0][s[free]] = vals[free]
            out[1][-1 - s[~free]] = vals[~free]
            return out

        xf, xfix = table(coords.numpy(), x_src, xfree)
        uf, ufix = table(u.numpy(), u_src, ufree)
        conn_x = np.asarray(x_src)[conn.numpy()].astype(np.int32)
        path = str(tmp_path / f"{kind}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<8q", conn.shape[0], npe, n_u, len(a_col), len(host.arr(-1, 1)), len(xf), len(xfix), len(ufix)))
            f.write(struct.pack("<3d", lam, mu, W))
            for a in (conn_x, host.arr(-1, 4), host.arr(-1, 0), host.arr(-1, 1), host.arr(-1, 2), host.arr(-1, 3), a_ptr):
                f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
            for a in (xf, xfix, uf, ufix, want):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        out = subprocess.run([exe, path], capture_output=True, text=True)
        print(kind, out.stdout.strip())
        assert out.returncode == 0, out.stdout + out.stderr
        assert " 0 Dirichlet columns" not in out.stdout
