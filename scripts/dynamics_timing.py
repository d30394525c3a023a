#!/usr/bin/env python3
"""Implicit dynamics at T1M / Q1M (dev tool; gates nothing): the 10^6-element TRI3 (1001 x 501 nodes) and, with `--quad`, QUAD4
(1415 x 708 nodes) benchmark meshes, left edge clamped, fp64, physical convention, rho = 2, consistent mass
(hidenn_fem_amd/dynamics.py, the MASS instances of csrc/tri3_cg.hip and csrc/quad4_cg.hip, csrc/dynamics.hip).

One JSON object -> `profiles/dynamics/dynamics_timing_{T1M,Q1M}.json`:
  * `apply`: the shifted apply q = (c_K K + c_M M) p against the plain apply q = K p on the same plan, and their ratio -- the
    claim "the mass term is free inside the apply"  is this number; the separate mass apply for comparison;
  * `setup`: the 2x2 block diagonal (per setup call, plain and shifted timed in alternating windows) and the AMG numeric setup (wall time, host inverse of the coarsest level
    included, median of 5), shifted against plain;
  * `vector`: the three Newmark vector kernels with their algorithmic bytes and the time those take at 8 TB/s;
  * `steps`: CG iterations and wall time per step over `--steps` steps of a step load from rest at dt = T1 / 20 and T1 / 400
    for `amg` and `block_jacobi` (rtol 1e-10); T1 from `ModalSolver` (one mode).
Launch times: device events around back-to-back launches on preallocated buffers, median of 5 runs.  Cache regime: the same
buffers every call; a vector is 8 MB at T1M, so the vector kernels' working set (40-48 MB) sits in the 256 MB Infinity Cache.

    python scripts/dynamics_timing.py [--quad] [--reps 20] [--steps 3] [--out-dir profiles/dynamics] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.dynamics import NewmarkSolver
from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.modal import ModalSolver
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D

F64 = torch.float64
HBM_BYTES_PER_US = 8e6          # 8 TB/s
RHO = 2.0


def events_us(fn, reps):
    """Mean device time per call of `fn` over `reps` back-to-back calls (after a warm-up), median of 5 such runs."""
    for _ in range(2):
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


def events_pair_us(fa, fb, reps):
    """`events_us` for two callables timed in ALTERNATING windows (a, b, a, b, ...), so both see the same clock regime."""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(5):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / reps)
    return median(out[0]), median(out[1])


def entry(us, nbytes):
    return dict(us=us, algorithmic_bytes=nbytes, us_at_8TBps=nbytes / HBM_BYTES_PER_US,
                times_the_byte_bound=us / (nbytes / HBM_BYTES_PER_US))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def measure(name, quad, nx, ny, reps, n_steps):
    dev = torch.device("cuda:0")
    mesher, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)

    def model():
        m = cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
        with torch.no_grad():
            m.u_free.zero_()
        return m

    lf = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    m = model()
    lam1 = float(ModalSolver(m, lf, n_modes=1, density=RHO, precond="amg", rtol=1e-8).solve().eigenvalues[0])
    T1 = 2.0 * 3.141592653589793 / lam1 ** 0.5
    s = NewmarkSolver(m, lf, T1 / 20.0, density=RHO, precond="amg")
    s.refresh()
    n, ln, L, st = s.n_u, s.len, _lib.lib(), _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    v = [torch.randn((n, 2), dtype=F64, device=dev, generator=g) for _ in range(9)]
    p = _lib.ptr
    vec = 16 * n
    plain = events_us(lambda: s._apply_k(v[0], v[1]), reps)
    shifted = events_us(lambda: s._apply_a(v[0], v[1]), reps)
    mass = events_us(lambda: s._apply_m(v[0], v[1]), reps)
    apply = dict(plain_us=plain, shifted_us=shifted, shifted_over_plain=shifted / plain, separate_mass_apply_us=mass,
                 composed_over_plain=(plain + mass) / plain)
    mat, W = s._mat()
    xf, xfix = s.solver._xf, s.solver._xfix

    def plain_diag():
        _lib.check(L.hfem_cg_setup(s.solver._h, p(xf), p(xfix) if xfix.numel() else None, mat, W, 1, p(s.solver.diag), st))

    amg_plain, amg_shifted = [], []
    for _ in range(5):
        s._amg.setup(xf, xfix, mat, W)
        amg_plain.append(s._amg.seconds)
        s._amg.setup_shifted(xf, xfix, mat, W, s.c_k, s.c_m * RHO, False)
        amg_shifted.append(s._amg.seconds)
    diag_plain, diag_shifted = events_pair_us(plain_diag, lambda: s._bind(s.c_k, s.c_m), reps)
    setup = dict(block_diagonal_plain_us=diag_plain, block_diagonal_shifted_us=diag_shifted,
                 block_diagonal_note="per setup call, alternating windows: one launch plus the entry point's host walk over the "
                                     "plan's row map, so back-to-back calls can be host-bound",
                 amg_numeric_plain_ms=1e3 * median(amg_plain), amg_numeric_shifted_ms=1e3 * median(amg_shifted))
    _lib.check(L.hfem_cg_setup(s.solver._h, p(xf), p(xfix) if xfix.numel() else None, mat, W, 0, p(s.solver.diag), st))
    vector = dict(
        predict=entry(events_us(lambda: _lib.check(L.hfem_newmark_predict(0, p(v[0]), p(v[1]), p(v[2]), ln, 0.1, 0.25, 0.5, 0.01,
                                                                          p(v[3]), p(v[4]), p(v[5]), st)), reps), 6 * vec),
        rhs=entry(events_us(lambda: _lib.check(L.hfem_newmark_rhs(0, p(v[0]), p(v[1]), p(v[2]), p(v[3]), ln, 1.0, 0.1, p(v[4]),
                                                                  p(v[5]), st)), reps), 6 * vec),
        rhs_without_mass_term=entry(events_us(lambda: _lib.check(L.hfem_newmark_rhs(0, p(v[0]), p(v[1]), None, p(v[3]), ln, 1.0,
                                                                                    0.0, p(v[4]), p(v[5]), st)), reps), 5 * vec),
        correct=entry(events_us(lambda: _lib.check(L.hfem_newmark_correct(0, p(v[3]), p(v[4]), p(v[2]), ln, 0.1, 0.25, 0.5,
                                                                          p(v[6]), p(v[7]), st)), reps), 5 * vec))
    del s
    steps = {}
    for frac in (20, 400):
        for precond in ("amg", "block_jacobi"):
            sv = NewmarkSolver(model(), lf, T1 / frac, density=RHO, precond=precond, max_iter=20000)
            sv.set_state()
            its, wall = [], []
            for _ in range(n_steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = sv.step(1)[0]
                torch.cuda.synchronize()
                wall.append(time.perf_counter() - t0)
                its.append(info.iterations if info.converged else -info.iterations)
            steps[f"T1/{frac} {precond}"] = dict(iterations=its, wall_ms=[1e3 * w for w in wall],
                                                 amg=None if sv._amg is None else sv._amg.report())
            del sv
    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2, left edge clamped",
                n_elems=m.Nelems, n_nodes=m.Nnodes, free_dofs=2 * n, density=RHO, mass="consistent", T1=T1,
                timing="device events around back-to-back launches on preallocated buffers, median of 5 runs",
                apply=apply, setup=setup, vector=vector, steps=steps,
                steps_note="iterations per step (negative: not converged within max_iter 20000), wall per step() call with "
                           "its host synchronisations; rtol 1e-10, warm start from the previous a")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--quad", action="store_true", help="Q1M instead of T1M")
    ap.add_argument("--small", action="store_true", help="101x51 / 142x71 nodes (a check that the script runs)")
    a = ap.parse_args()
    name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
    if a.small:
        nx, ny = nx // 10 + 1, ny // 10 + 1
    line = json.dumps(measure(name, quad, nx, ny, a.reps, a.steps))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"dynamics_timing_{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
