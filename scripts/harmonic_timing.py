#!/usr/bin/env python3
"""Harmonic response at T1M / Q1M (dev tool; gates nothing): the 10^6-element TRI3 (1001 x 501 nodes) and, with `--quad`, QUAD4
(1415 x 708 nodes) benchmark meshes, left edge clamped, fp64, physical convention, rho = 2, consistent mass
(hidenn_fem_amd/harmonic.py, csrc/harmonic.hip).

One JSON object -> `profiles/harmonic/harmonic_timing_{T1M,Q1M}.json`:
  * `apply`: the complex apply q = (z_K K + z_M M) p on a complex vector against the real shifted apply q = (c_K K + c_M M) p
    (`hfem_cg_apply` after `hfem_cg_setup_shifted`: the MASS instance) and the plain apply q = K p, all on the same plan, and
    the ratios.  The design argument is a ratio well under 2: indices and coordinates are shared, the arithmetic
    and the LDS atomics double.  The ratio is recorded, not tuned to;
  * `iteration`: one COCG iteration with each preconditioner (a captured graph of `--iters` iterations, restarted before every
    replay so that no replayed iteration has halted);
  * `solve`: iterations and wall time of the three frequencies omega_1 / 2, sqrt(omega_2 omega_3), omega_1 with 2 % Rayleigh
    damping at omega_1 and omega_3, each from a zero start, per preconditioner (`--solve-preconds`).
Launch times: hipGraph replay of `--reps` back-to-back launches on preallocated buffers between device events, median of
`--samples` replays after two warm-up replays.  Cache regime: the same buffers every launch; a complex vector is 16 MB at T1M,
so vectors sit in the 256 MB Infinity Cache while the plan's index arrays stream.

    python scripts/harmonic_timing.py [--quad] [--reps 20] [--samples 7] [--iters 8] [--out-dir profiles/harmonic] [--small]
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
from hidenn_fem_amd.harmonic import HarmonicSolver
from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.modal import ModalSolver
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D

F64 = torch.float64
RHO, ZETA = 2.0, 0.02


def median(xs):
    return sorted(xs)[len(xs) // 2]


def graph_us(fn, reps, samples, before=None):
    """Median device time per call of `fn`: `reps` calls captured in one graph, `samples` timed replays after two warm-up
    replays; `before()` runs (untimed) ahead of every replay."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    out = []
    for k in range(samples + 2):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            out.append(a.elapsed_time(b) * 1e3 / reps)
    return median(out), out


def measure(name, quad, nx, ny, reps, samples, iters, solve_preconds, max_iter):
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
    lam = ModalSolver(m, lf, n_modes=3, density=RHO, precond="amg", rtol=1e-8).solve().eigenvalues
    w1, w2, w3 = (float(lam[j]) ** 0.5 for j in range(3))
    ray = (2.0 * ZETA * w1 * w3 / (w1 + w3), 2.0 * ZETA / (w1 + w3))
    omegas = [0.5 * w1, (w2 * w3) ** 0.5, w1]
    L = _lib.lib()
    p = _lib.ptr
    # ---- apply: complex against the real shifted and the plain apply of the same plan
    nm = NewmarkSolver(m, lf, 1.0 / w1, density=RHO, precond="block_jacobi")
    nm.refresh()
    hs = HarmonicSolver(m, lf, density=RHO, rayleigh=ray, precond="none")
    hs.refresh()
    hs._bind(omegas[1])
    assert hs.solver.plan is nm.solver.plan
    n = hs.n_u
    g = torch.Generator(device=dev).manual_seed(0)
    P, Q = torch.randn((2, n, 2), dtype=F64, device=dev, generator=g), torch.empty((2, n, 2), dtype=F64, device=dev)
    pq = torch.empty(2, dtype=F64, device=dev)
    t_plain, _ = graph_us(lambda: nm._apply_k(P[0], Q[0]), reps, samples)
    t_shift, s_shift = graph_us(lambda: nm._apply_a(P[0], Q[0]), reps, samples)
    # the stream is looked up at every call: inside a capture the current stream is the capturing one
    t_cplx, s_cplx = graph_us(lambda: _lib.check(L.hfem_harm_apply(hs._h, p(P), p(Q), hs.len, p(pq), _lib.stream_ptr(dev))), reps,
                              samples)
    apply = dict(plain_us=t_plain, shifted_us=t_shift, complex_us=t_cplx, complex_over_shifted=t_cplx / t_shift,
                 complex_over_plain=t_cplx / t_plain, shifted_samples_us=s_shift, complex_samples_us=s_cplx,
                 tile=dict(hs.solver.plan.stats), lds_bytes=48 * hs.solver.plan.stats["max_tile_nodes"] +
                 32 * hs.solver.plan.stats["max_tile_owned"] + 8 * (2 * (hs.solver.plan.stats["threads_per_tile"] // 64) + 2))
    del nm, hs
    # ---- one COCG iteration per preconditioner
    iteration = {}
    for precond in ("none", "block_jacobi", "amg"):
        s = HarmonicSolver(m, lf, density=RHO, rayleigh=ray, precond=precond, iters_per_graph=iters)
        s.refresh()
        s._set_rhs(None)
        s._bind(omegas[1])
        s._build_precond(omegas[1])
        amg = s._amg._h if s._amg is not None else None
        diag = p(s.diag) if precond == "block_jacobi" else None

        def restart():
            s._x.zero_()
            _lib.check(L.hfem_harm_start(s._h, amg, diag, p(s._b), None, s.len, 0.0, 0.0, 1 << 40, _lib.stream_ptr(dev)))

        restart()
        t_it, samp = graph_us(s._iterate, 1, samples, before=restart)
        status = s._read_status()
        iteration[precond] = dict(us_per_iteration=t_it / iters, iterations_per_graph=iters, samples_us=[v / iters for v in samp],
                                  halted_after_the_last_replay=bool(status[10]), iterations_after_the_last_replay=int(status[0]))
        del s
    # ---- the three-frequency solve
    solve = {}
    for precond in solve_preconds:
        s = HarmonicSolver(model(), lf, density=RHO, rayleigh=ray, precond=precond, rtol=1e-8, max_iter=max_iter)
        rows = []
        for w in omegas:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info = s.solve(w)
            torch.cuda.synchronize()
            rows.append(dict(omega=w, omega_over_omega_1=w / w1, iterations=info.iterations, reason=info.reason,
                             relative_residual=info.residual / info.rhs_norm, wall_ms=1e3 * (time.perf_counter() - t0)))
        solve[precond] = dict(frequencies=rows, amg=None if s._amg is None else s._amg.report())
        del s
    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2, left edge clamped",
                n_elems=m.Nelems, n_nodes=m.Nnodes, free_dofs=2 * n, density=RHO, mass="consistent", omega_1_2_3=[w1, w2, w3],
                rayleigh=ray, zeta=ZETA,
                timing=f"hipGraph replay of {reps} launches between device events, median of {samples} replays after 2 warm-ups",
                apply=apply, iteration=iteration, solve=solve,
                solve_note=f"rtol 1e-8, zero start, max_iter {max_iter}; wall per solve() call with its host synchronisations, "
                           "the preconditioner setup at the frequency and (first frequency) the graph capture included")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--solve-preconds", default="amg", help="comma-separated: amg, block_jacobi, none")
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--quad", action="store_true", help="Q1M instead of T1M")
    ap.add_argument("--small", action="store_true", help="101x51 / 142x71 nodes (a check that the script runs)")
    a = ap.parse_args()
    name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
    if a.small:
        nx, ny = nx // 10 + 1, ny // 10 + 1
    line = json.dumps(measure(name, quad, nx, ny, a.reps, a.samples, a.iters, [s for s in a.solve_preconds.split(",") if s],
                              a.max_iter))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"harmonic_timing_{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
