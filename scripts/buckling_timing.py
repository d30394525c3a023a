#!/usr/bin/env python3
"""The buckling solver at T1M / Q1M (dev tool; gates nothing): the 10^6-element TRI3 (1001 x 501 nodes) and, with `--quad`, QUAD4
(1415 x 708 nodes) benchmark meshes, left edge clamped, the default traction reversed into compression, fp64, physical convention
(hidenn_fem_amd/buckling.py, csrc/buckling.hip).

One JSON object -> `profiles/buckling/buckling_timing_{T1M,Q1M}.json`:
  * `launch`: device time per call of the geometric-stiffness setup (one launch per prestress state), of the K_G apply at 8
    columns and of `hfem_mass_apply` (consistent, 8 columns) on the same mesh -- the mass kernel has the same frame (one thread
    per free row walking the node's element fan) and is the yardstick: `geom_over_mass` is the ratio of the two.  Device events
    around back-to-back calls on preallocated buffers, median of 5 runs, with the algorithmic bytes of each (every array read or
    written once) and the time they take at 8 TB/s;
  * `iteration`: one LOBPCG iteration's pieces at the solve's block width, timed the same way: the K_G apply, the `block` K
    applies, the `block` V-cycles (or the one block-Jacobi launch) and the block-vector kernels (residual, two Grams, three
    combines);
  * `static`: CG iterations and wall time of the static solve that gives the prestress;
  * `solve`: iterations and wall time of `solve()` to `rtol = 1e-8` for four modes with `--precond` (default amg), host
    synchronisation and host Ritz steps included.
Cache regime: back-to-back launches on the same buffers.

    python scripts/buckling_timing.py [--quad] [--precond amg|block_jacobi] [--reps 10] [--out-dir profiles/buckling] [--small]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.buckling import BucklingSolver
from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.modal import MAX_BLOCK, ModalSolver
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
from hidenn_fem_amd.solve import solve_displacement_

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
    lf = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical", gauss_order=1)
    with torch.no_grad():
        m.u_free.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = solve_displacement_(m, lf, t_force=lambda x: -lf.uniform_edge_force(x), precond=precond, rtol=1e-10)
    torch.cuda.synchronize()
    static = dict(precond=precond, rtol=1e-10, iterations=st.iterations, reason=st.reason, wall_seconds=time.perf_counter() - t0)
    s = BucklingSolver(m, lf, n_modes=4, precond=precond, rtol=1e-8, max_iter=200 if precond == "amg" else 20000)
    mass = ModalSolver(m, lf, n_modes=4, precond="block_jacobi")           # the yardstick: hfem_mass_apply on the same mesh
    s._refresh()
    mass._refresh()
    b, n, ln = s.block, s.n_u, s.len
    g = torch.Generator(device=dev).manual_seed(0)
    S, KS, MS = (torch.randn((3 * MAX_BLOCK, n, 2), dtype=F64, device=dev, generator=g) for _ in range(3))
    O = torch.empty((2 * MAX_BLOCK, n, 2), dtype=F64, device=dev)
    s._coef.copy_(torch.randn(s._coef.shape, dtype=F64, device=dev, generator=g))
    ne, nn, npe = m.Nelems, m.Nnodes, conn.shape[1]
    vec = 16 * n                                                           # bytes of one vector

    def setup():
        s._geom_key = None
        s._refresh()

    def block_kernels():
        s._residual_into(KS, MS, S[2 * b:], b)
        s._grams(S, KS, MS, 3 * b)
        for a in (S, KS, MS):
            _lib.check(_lib.lib().hfem_block_combine(0, _lib.ptr(a), 3 * b, _lib.ptr(s._coef), 2 * b, ln, _lib.ptr(O), _lib.stream_ptr(dev)))

    fan = 4 * (nn + 1) + 4 * npe * ne + 8 * n                              # adjacency pointers and entries, row_node, node_row
    geom_bytes = fan + 4 * npe * ne + 8 * npe * npe * ne + 2 * MAX_BLOCK * vec
    mass_bytes = fan + 4 * npe * ne + 16 * nn + 2 * MAX_BLOCK * vec
    setup_bytes = 4 * npe * ne + 16 * nn + vec + 8 * nn + 8 * npe * npe * ne
    launch = dict(
        geom_setup=entry(events_us(setup, reps), setup_bytes, 1),
        geom_apply_8=entry(events_us(lambda: s._geom_into(S, KS, MAX_BLOCK), reps), geom_bytes, 1),
        mass_apply_consistent_8=entry(events_us(lambda: mass._mass_into(S, KS, MAX_BLOCK), reps), mass_bytes, 1))
    launch["geom_over_mass"] = launch["geom_apply_8"]["us"] / launch["mass_apply_consistent_8"]["us"]
    iteration = dict(block=b,
                     geom_apply=events_us(lambda: s._geom_into(S, KS, b), reps),
                     k_applies=events_us(lambda: s._stiffness_into(S, MS, b), reps),
                     preconditioner=events_us(lambda: s._precondition_into(S[:b], S[b:2 * b], b), reps),
                     block_kernels=events_us(block_kernels, reps))
    iteration["geom_apply_share"] = iteration["geom_apply"] / sum(iteration[k] for k in ("geom_apply", "k_applies", "preconditioner",
                                                                                          "block_kernels"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2, left edge clamped, default traction "
                     "reversed", n_elems=ne, n_nodes=nn, free_dofs=2 * n, precond=precond,
                timing="device events around back-to-back launches on preallocated buffers, median of 5 runs",
                launch=launch, iteration=iteration, static=static,
                solve=dict(n_modes=4, block=b, rtol=1e-8, iterations=info.iterations, converged=info.converged, restarts=s.restarts,
                           n_buckling=info.n_buckling, wall_seconds=wall, ms_per_iteration=1e3 * wall / max(info.iterations + 1, 1),
                           load_factors=info.load_factors.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--quad", action="store_true", help="Q1M instead of T1M")
    ap.add_argument("--precond", choices=["amg", "block_jacobi"], default="amg")
    ap.add_argument("--small", action="store_true", help="101x51 / 142x71 nodes (a check that the script runs)")
    a = ap.parse_args()
    name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
    if a.small:
        nx, ny = nx // 10 + 1, ny // 10 + 1
    line = json.dumps(measure(name, quad, nx, ny, a.reps, a.precond))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"buckling_timing_{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
