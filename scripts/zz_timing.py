#!/usr/bin/env python3
"""Nodal stress recovery and ZZ error estimate at T1M and Q1M (dev tool; gates nothing): the 10^6-element TRI3 (1001 x 501
nodes) and QUAD4 (1415 x 708 nodes) benchmark meshes, fp64, physical convention (hidenn_fem_amd/post.py, csrc/recover.hip).

Per mesh, as one JSON object:
  * `recover`: the stress_recover launch; `error`: the zz_error launch + its one-block finish -- device events around
    back-to-back calls on preallocated buffers, median of 5 runs;
  * `torch_recover` / `torch_error`: the same quantities composed from torch ops on the GPU (gathers, element-wise closed
    forms, `index_add_`, which accumulates with atomics: neither ordered nor reproducible), same timing;
  * the algorithmic bytes of each (every array read or written once) and the time they take at 8 TB/s.
The node walk of `recover` is a chain of four dependent gathers (adjacency -> connectivity -> node rows -> arithmetic) per
adjacent element, like the deterministic energy path: L2-latency bound, far from the byte bound.  Cache regime: the working
sets stay in the 256 MB Infinity Cache.

    python scripts/zz_timing.py [--reps 20] [--out-dir profiles/zz]

`--neo-hookean [--quad]`: the finite-strain twins (`HyperStressRecovery`, the Cauchy law in the same kernels) at
T1M (with `--quad`: Q1M) on a smooth finite-strain field with min det F about 0.5, and, in the same run on the same mesh and
displacement, the linear launches: `hyper_recover` / `hyper_error` and `linear_recover` / `linear_error` timed as above, each
Neo-Hookean-to-linear ratio and the algorithmic bytes -> `hyper_zz_timing_{T1M,Q1M}.json`.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
from hidenn_fem_amd.post import HyperStressRecovery, StressRecovery

F64 = torch.float64
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def events_us(fn, reps):
    """Mean device time per call of `fn` over `reps` back-to-back calls (after a warm-up), median of 5 such runs."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(out)[len(out) // 2]


def field(x):
    return 1e-4 * torch.stack([torch.sin(2.1 * x[:, 0]) * torch.cos(1.3 * x[:, 1]),
                               0.5 * torch.cos(1.7 * x[:, 0] + 0.3) * torch.sin(2.4 * x[:, 1])], dim=1)


def torch_points(X, U, conn, mat):
    """Physical-convention sigma_h [Ne, NQ, 3], weights [Ne, NQ] and shape values [NQ, npe] from torch ops."""
    npe = conn.shape[1]
    Xe, Ue = X[conn], U[conn]                                            # [Ne, npe, 2]
    if npe == 3:
        D = torch.tensor([[[1.0, 0.0, -1.0], [0.0, 1.0, -1.0]]], dtype=F64, device=X.device)          # [1, 2, 3]
        N = torch.full((1, 3), 1.0 / 3.0, dtype=F64, device=X.device)
        wf = 0.5
    else:
        g = 3.0 ** -0.5
        xi = torch.tensor([-g, g, -g, g], dtype=F64, device=X.device)[:, None]
        eta = torch.tensor([-g, -g, g, g], dtype=F64, device=X.device)[:, None]
        xk = torch.tensor([-1.0, 1.0, 1.0, -1.0], dtype=F64, device=X.device)[None, :]
        ek = torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=F64, device=X.device)[None, :]
        D = torch.stack([0.25 * xk * (1 + ek * eta), 0.25 * ek * (1 + xk * xi)], dim=1)               # [4, 2, 4]
        N = 0.25 * (1 + xk * xi) * (1 + ek * eta)
        wf = 1.0
    J = torch.einsum("eki,qjk->eqij", Xe, D)                             # J[i][j] = d x_i / d xi_j
    G = torch.einsum("eki,qjk->eqij", Ue, D)
    det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    Jinv = torch.stack([torch.stack([J[..., 1, 1], -J[..., 0, 1]], -1), torch.stack([-J[..., 1, 0], J[..., 0, 0]], -1)], -2) / det[..., None, None]
    H = G @ Jinv                                                         # physical convention
    exx, eyy, gam = H[..., 0, 0], H[..., 1, 1], H[..., 0, 1] + H[..., 1, 0]
    sig = torch.stack([mat[0] * exx + mat[1] * eyy, mat[1] * exx + mat[2] * eyy, mat[3] * gam], -1)
    return sig, wf * det.abs(), N


def torch_recover(X, U, conn, mat):
    sig, w, N = torch_points(X, U, conn, mat)
    wn = w[:, :, None] * N[None]
    num = torch.zeros(X.shape[0], 3, dtype=F64, device=X.device).index_add_(0, conn.reshape(-1), torch.einsum("eqk,eqi->eki", wn, sig).reshape(-1, 3))
    den = torch.zeros(X.shape[0], dtype=F64, device=X.device).index_add_(0, conn.reshape(-1), wn.sum(1).reshape(-1))
    return num / den[:, None]


def torch_error(X, U, conn, mat, star):
    sig, w, N = torch_points(X, U, conn, mat)
    D = mat[0] * mat[2] - mat[1] * mat[1]
    S = torch.tensor([[mat[2] / D, -mat[1] / D, 0.0], [-mat[1] / D, mat[0] / D, 0.0], [0.0, 0.0, 1.0 / mat[3]]], dtype=F64, device=X.device)
    form = lambda d: torch.einsum("...i,ij,...j->...", d, S, d)
    ss = star[conn]
    if conn.shape[1] == 3:
        d = ss - sig
        eta2 = w[:, 0] / 12.0 * (form(d).sum(1) + form(d.sum(1)))
    else:
        eta2 = (w * form(torch.einsum("qk,eki->eqi", N, ss) - sig)).sum(1)
    return eta2, eta2.sum(), (w * form(sig)).sum()


def measure(name, quad, nx, ny, reps):
    dev = torch.device("cuda:0")
    mesher = structured_quad_mesh if quad else structured_tri_mesh
    coords, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    m = PiecewiseLinearShapeNN2D(coords, conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(field(coords), "u"))
    m = m.to(dev)
    lf = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    sr = StressRecovery(m, lf)
    ne, nn, npe = m.Nelems, m.Nnodes, conn.shape[1]
    _, X, U, flags = sr._inputs()
    sig = torch.empty(nn, 3, dtype=F64, device=dev)
    eta2 = torch.empty(ne, dtype=F64, device=dev)
    totals = torch.zeros(2, dtype=F64, device=dev)
    L, di, st, p = _lib.lib(), _lib.dev_index(dev), _lib.stream_ptr(dev), _lib.ptr
    kind = "quad4" if quad else "tri3"
    rec_fn, zz_fn = getattr(L, f"hfem_{kind}_stress_recover"), getattr(L, f"hfem_{kind}_zz_error")
    mat = (C.c_double * 4)(*lf._mat)

    def recover():
        _lib.check(rec_fn(di, p(X), p(U), p(m._conn32), ne, nn, p(sr._adj_ptr), p(sr._adj), mat, flags, p(sig), None, st))

    def error():
        _lib.check(zz_fn(di, p(X), p(U), p(m._conn32), ne, p(sig), mat, flags, p(eta2), None, p(sr._partials), p(totals), st))

    recover()
    error()
    connl = m.connectivity
    star = torch_recover(X, U, connl, lf._mat)
    t_eta2, t_e, t_n = torch_error(X, U, connl, lf._mat, sig)
    e2, n2 = totals.tolist()
    agree = dict(nodal_stress=((star - sig).abs().max() / sig.abs().max()).item(), eta2=((t_eta2 - eta2).abs().max() / eta2.max()).item(),
                 eta2_total=abs(t_e.item() - e2) / e2, norm2_total=abs(t_n.item() - n2) / n2)
    rec_bytes = 4 * (nn + 1) + 2 * 4 * npe * ne + 32 * nn + 24 * nn
    err_bytes = 4 * npe * ne + 32 * nn + 24 * nn + 8 * ne
    r_us, e_us = events_us(recover, reps), events_us(error, reps)
    tr_us = events_us(lambda: torch_recover(X, U, connl, lf._mat), max(reps // 4, 2))
    te_us = events_us(lambda: torch_error(X, U, connl, lf._mat, sig), max(reps // 4, 2))
    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2", n_elems=ne, n_nodes=nn,
                convention="physical", eta_rel=(e2 / (n2 + e2)) ** 0.5,
                regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)",
                recover=dict(us=r_us, launches=1, algorithmic_bytes=rec_bytes, us_at_8TBps=rec_bytes / HBM_BYTES_PER_US,
                             times_the_byte_bound=r_us / (rec_bytes / HBM_BYTES_PER_US)),
                error=dict(us=e_us, launches=2, algorithmic_bytes=err_bytes, us_at_8TBps=err_bytes / HBM_BYTES_PER_US,
                           times_the_byte_bound=e_us / (err_bytes / HBM_BYTES_PER_US)),
                torch_recover=dict(us=tr_us, over_kernel=tr_us / r_us), torch_error=dict(us=te_us, over_kernel=te_us / e_us),
                torch_vs_kernel_max_rel=agree)


def finite_field(x, scale=0.66):
    """A smooth finite-strain field: min det F about 0.5, max about 1.65 on the jittered benchmark meshes."""
    return scale * torch.stack([0.25 * torch.sin(2.1 * x[:, 0]) * torch.cos(1.3 * x[:, 1]),
                                0.15 * torch.cos(1.7 * x[:, 0] + 0.3) * torch.sin(2.4 * x[:, 1])], dim=1)


def measure_hyper(name, quad, nx, ny, reps):
    from hidenn_fem_amd.loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    dev = torch.device("cuda:0")
    mesher = structured_quad_mesh if quad else structured_tri_mesh
    coords, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    m = PiecewiseLinearShapeNN2D(coords, conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(finite_field(coords), "u"))
    m = m.to(dev)
    lf = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    hf = (Quad4NeoHookeanLoss2D if quad else NeoHookeanLoss2D)(device=dev, dtype=F64)
    sr, hr = StressRecovery(m, lf), HyperStressRecovery(m, hf)
    ne, nn, npe = m.Nelems, m.Nnodes, conn.shape[1]
    _, X, U, flags = sr._inputs()
    sig, hsig = (torch.empty(nn, 3, dtype=F64, device=dev) for _ in range(2))
    eta2, heta2 = (torch.empty(ne, dtype=F64, device=dev) for _ in range(2))
    totals, htotals = torch.zeros(2, dtype=F64, device=dev), torch.zeros(4, dtype=F64, device=dev)
    L, di, st, p = _lib.lib(), _lib.dev_index(dev), _lib.stream_ptr(dev), _lib.ptr
    kind = "quad4" if quad else "tri3"
    rec_fn, zz_fn = getattr(L, f"hfem_{kind}_stress_recover"), getattr(L, f"hfem_{kind}_zz_error")
    hrec_fn, hzz_fn = getattr(L, f"hfem_{kind}_hyper_stress_recover"), getattr(L, f"hfem_{kind}_hyper_zz_error")
    mat, lame = (C.c_double * 4)(*lf._mat), (C.c_double * 2)(*hf.lame)

    def recover():
        _lib.check(rec_fn(di, p(X), p(U), p(m._conn32), ne, nn, p(sr._adj_ptr), p(sr._adj), mat, flags, p(sig), None, st))

    def error():
        _lib.check(zz_fn(di, p(X), p(U), p(m._conn32), ne, p(sig), mat, flags, p(eta2), None, p(sr._partials), p(totals), st))

    def hyper_recover():
        _lib.check(hrec_fn(di, p(X), p(U), p(m._conn32), ne, nn, p(hr._adj_ptr), p(hr._adj), lame, p(hsig), None, None, st))

    def hyper_error():
        _lib.check(hzz_fn(di, p(X), p(U), p(m._conn32), ne, p(hsig), lame, p(heta2), None, p(hr._partials), p(htotals), st))

    for fn in (recover, error, hyper_recover, hyper_error):
        fn()
    e2, n2, min_j, count = htotals.tolist()
    le2, ln2 = totals.tolist()
    nb = (ne + 255) // 256
    rec_bytes = 4 * (nn + 1) + 2 * 4 * npe * ne + 32 * nn + 24 * nn          # adjacency, connectivity, X and U rows, sigma*
    err_bytes = 4 * npe * ne + 32 * nn + 24 * nn + 8 * ne                    # connectivity, rows, sigma*, eta2
    t = {k: events_us(fn, reps) for k, fn in (("linear_recover", recover), ("linear_error", error),
                                              ("hyper_recover", hyper_recover), ("hyper_error", hyper_error))}

    def entry(us, nbytes, launches):
        return dict(us=us, launches=launches, algorithmic_bytes=nbytes, us_at_8TBps=nbytes / HBM_BYTES_PER_US,
                    times_the_byte_bound=us / (nbytes / HBM_BYTES_PER_US))

    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2", n_elems=ne, n_nodes=nn,
                field="0.66 (0.25 sin 2.1x cos 1.3y, 0.15 cos(1.7x + 0.3) sin 2.4y)", min_J=min_j, inverted=int(count),
                eta_rel=(e2 / (n2 + e2)) ** 0.5, linear_eta_rel_same_displacement=(le2 / (ln2 + le2)) ** 0.5,
                timing="device events around back-to-back launches on preallocated buffers, median of 5 runs",
                regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)",
                hyper_recover=entry(t["hyper_recover"], rec_bytes, 1), hyper_error=entry(t["hyper_error"], err_bytes + 32 * nb, 2),
                linear_recover=entry(t["linear_recover"], rec_bytes, 1), linear_error=entry(t["linear_error"], err_bytes + 16 * nb, 2),
                hyper_over_linear=dict(recover=t["hyper_recover"] / t["linear_recover"], error=t["hyper_error"] / t["linear_error"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--small", action="store_true", help="101x51 / 143x72 meshes (a check that the script runs)")
    ap.add_argument("--neo-hookean", action="store_true", help="the finite-strain twins against the linear launches, T1M")
    ap.add_argument("--quad", action="store_true", help="with --neo-hookean: Q1M instead of T1M")
    a = ap.parse_args()
    if a.neo_hookean:
        name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
        if a.small:
            nx, ny = nx // 10 + 1, ny // 10 + 1
        line = json.dumps(measure_hyper(name, quad, nx, ny, a.reps))
        print(line)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"hyper_zz_timing_{name}.json"), "w") as f:
                f.write(line + "\n")
        return
    for name, quad, nx, ny in (("T1M", False, 1001, 501), ("Q1M", True, 1415, 708)):
        if a.small:
            nx, ny = nx // 10 + 1, ny // 10 + 1
        line = json.dumps(measure(name, quad, nx, ny, a.reps))
        print(line)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"zz_timing_{name}.json"), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
