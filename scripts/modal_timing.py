#!/usr/bin/env python3
"""The modal solver at T1M / Q1M (dev tool; gates nothing): the 10^6-element TRI3 (1001 x 501 nodes) and, with `--quad`, QUAD4
(1415 x 708 nodes) benchmark meshes, left edge clamped, fp64, physical convention (hidenn_fem_amd/modal.py, csrc/modal.hip).

One JSON object -> `profiles/modal/modal_timing_{T1M,Q1M}.json`:
  * `launch`: device time per call of mass apply (consistent and lumped, 8 columns), Gram (24 x 24: one of the two of an
    iteration), combine (24 -> 16: one of the three) and residual (8 columns, with its finish) at `block = 8` -- device events
    around back-to-back calls on preallocated buffers, median of 5 runs -- with the algorithmic bytes of each (every array read
    or written once) and the time they take at 8 TB/s;
  * `iteration`: one LOBPCG iteration's pieces timed the same way: the 8 `K` applies, the 8 V-cycles (or the one block-Jacobi
    launch) and the new kernels together (residual, mass of W, two Grams, three combines);
  * `solve`: iterations and wall time of `solve()` to `rtol = 1e-8` for six modes with `--precond` (default amg), host
    synchronisation and host Ritz steps included.
Cache regime: back-to-back launches on the same buffers; the basis of 24 vectors (8 MB each at T1M) fits the 256 MB Infinity
Cache only in part once KS and MS are counted.

    python scripts/modal_timing.py [--quad] [--precond amg|block_jacobi] [--reps 10] [--out-dir profiles/modal] [--small]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.modal import _G, MAX_BLOCK, ModalSolver
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D

F64 = torch.float64
HBM_BYTES_PER_US = 8e6          # 8 TB/s


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


def entry(us, nbytes, launches):
    return dict(us=us, launches=launches, algorithmic_bytes=nbytes, us_at_8TBps=nbytes / HBM_BYTES_PER_US,
                times_the_byte_bound=us / (nbytes / HBM_BYTES_PER_US))


def measure(name, quad, nx, ny, reps, precond):
    dev = torch.device("cuda:0")
    mesher, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    m = cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
    lf = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    s = ModalSolver(m, lf, n_modes=6, block=8, precond=precond, rtol=1e-8, max_iter=200 if precond == "amg" else 20000)
    s._refresh()
    b, n, ln = 8, s.n_u, s.len
    g = torch.Generator(device=dev).manual_seed(0)
    S, KS, MS = (torch.randn((3 * b, n, 2), dtype=F64, device=dev, generator=g) for _ in range(3))
    O = torch.empty((2 * b, n, 2), dtype=F64, device=dev)
    s._coef.copy_(torch.randn(s._coef.shape, dtype=F64, device=dev, generator=g))
    ne, nn, npe = m.Nelems, m.Nnodes, conn.shape[1]
    vec = 16 * n                                                           # bytes of one vector

    def mass(kind):
        s.mass = kind
        s._mass_into(S, KS, b)

    def gram():
        _lib.check(_lib.lib().hfem_block_gram(0, _lib.ptr(S), 3 * b, _lib.ptr(KS), 3 * b, ln, _lib.ptr(s._gram_partials),
                                              _lib.ptr(s._rec), _lib.stream_ptr(dev)))

    def combine():
        _lib.check(_lib.lib().hfem_block_combine(0, _lib.ptr(S), 3 * b, _lib.ptr(s._coef), 2 * b, ln, _lib.ptr(O), _lib.stream_ptr(dev)))

    def new_kernels():
        s._residual_into(KS, MS, S[2 * b:], b)
        s._mass_into(S[2 * b:], MS[2 * b:], b)
        s._grams(S, KS, MS, 3 * b)
        for a in (S, KS, MS):
            _lib.check(_lib.lib().hfem_block_combine(0, _lib.ptr(a), 3 * b, _lib.ptr(s._coef), 2 * b, ln, _lib.ptr(O), _lib.stream_ptr(dev)))

    mass_bytes = 4 * (nn + 1) + 2 * 4 * npe * ne + 16 * nn + 8 * n + 2 * b * vec
    launch = dict(
        mass_apply_consistent=entry(events_us(lambda: mass("consistent"), reps), mass_bytes, 1),
        mass_apply_lumped=entry(events_us(lambda: mass("lumped"), reps), mass_bytes, 1),
        gram_24x24=entry(events_us(gram, reps), 2 * 3 * b * vec, 2),
        combine_24_to_16=entry(events_us(combine, reps), (3 * b + 2 * b) * vec, 1),
        residual_8=entry(events_us(lambda: s._residual_into(KS, MS, S[2 * b:], b), reps), 3 * b * vec, 2))
    s.mass = "consistent"
    iteration = dict(k_applies_8=events_us(lambda: s._stiffness_into(S, KS, b), reps),
                     preconditioner=events_us(lambda: s._precondition_into(S[:b], S[b:2 * b], b), reps),
                     new_kernels=events_us(new_kernels, reps))
    iteration["new_kernels_share"] = iteration["new_kernels"] / sum(iteration.values())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2, left edge clamped", n_elems=ne,
                n_nodes=nn, free_dofs=2 * n, block=b, basis_vectors=_G, precond=precond,
                timing="device events around back-to-back launches on preallocated buffers, median of 5 runs",
                launch=launch, iteration=iteration,
                solve=dict(n_modes=6, rtol=1e-8, iterations=info.iterations, converged=info.converged, restarts=s.restarts,
                           wall_seconds=wall, ms_per_iteration=1e3 * wall / max(info.iterations + 1, 1),
                           frequencies=info.frequencies.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--quad", action="store_true", help="Q1M instead of T1M")
    ap.add_argument("--precond", choices=["amg", "block_jacobi"], default="amg")
    ap.add_argument("--small", action="store_true", help="101x51 / 142x71 nodes (a check that the script runs)")
    a = ap.parse_args()
    assert MAX_BLOCK == 8
    name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
    if a.small:
        nx, ny = nx // 10 + 1, ny // 10 + 1
    line = json.dumps(measure(name, quad, nx, ny, a.reps, a.precond))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"modal_timing_{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
