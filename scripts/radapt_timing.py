#!/usr/bin/env python3
"""r-adaptive solve at T1M (dev tool): 10^6 TRI3, fp64, default traction (hidenn_fem_amd/radapt.py, csrc/mesh_guard.hip).
--quad: the same records for 10^6 QUAD4 cells (Quad4RAdaptiveSolver).

Records, as one JSON object:
  * the step-bound launch (init + element kernel), the measure launch (init + element kernel + finish), the barrier launch
    (zero fill of the value and the [n_x, 2] gradient + element kernel): device events around graph replays of 16 calls;
  * the graded energy evaluation on the same mesh (value_and_grad_), for scale;
  * one line-search trial (write x + a d, loss-only energy, host read of the value) and the coordinate gradient
    (loss_fn + autograd.grad on node_coords_free): host clock, synchronised, median of repeats;
  * three outer iterations of RAdaptiveSolver: per iteration the warm-started CG solve and everything else (host clock);
  * the 36 k-element example-4 plate (200 x 100, fp64), without and with the quality barrier (weight 0.05): outer iterations,
    Pi* before and after, reason, min q, wall time (--quad: the plate without holes, 200 x 100 nodes of QUAD4 cells).
Cache regime: the working sets stay in the 256 MB Infinity Cache.

--neo-hookean [--quad]: the finite-strain guard (HyperRAdaptiveSolver / Quad4HyperRAdaptiveSolver) on the same meshes, at a
smooth displacement field with min J about 0.5:
  * the fused det F-safe bound launch (init + element kernel);
  * the composition available without it -- the torch add that forms X + u on the coordinate rows, `hfem_*_step_bound` on X
    and on X + u, and the minimum of the two (the rows of u gathered onto the coordinate rows beforehand, not timed).  It
    bounds detJ(X) and detJ(X + u) separately, which is the weaker guarantee: det F = detJ(X + u) / detJ(X) keeps eta of its
    value only where the reference element does not grow along the step;
  * the deformation measure launch, without and with the per-element output;
  * --outer N outer iterations of the finite-strain solver under a downward traction (E = 2e6, --precond for Newton):
    per iteration the Newton solve and everything else (host clock), and the share spent outside Newton (0 skips this).
--lib FILE: load that build of the library instead of the tree's own (A/B of two builds with one ABI under the same driver).
--pieces: the mesh-kernel launches only (bound, measure, barrier; --neo-hookean: fused and composed bound, deformation
measure) on the mesh classes of radapt.py, no solver built and none of the solves.

    python scripts/radapt_timing.py [--grid 1001x501] [--reps 200] [--out profiles/radapt/radapt_timing_T1M.json]
    python scripts/radapt_timing.py --quad [--grid 1415x708] [--out profiles/radapt/radapt_timing_quad4_T1M.json]
    python scripts/radapt_timing.py --neo-hookean [--quad] [--outer 3] [--precond amg]
                                    [--out profiles/radapt/hyper_radapt_timing_T1M.json | ..._Q1M.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import generate_mesh, structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
from hidenn_fem_amd.radapt import Quad4RAdaptiveSolver, RAdaptiveSolver, mesh_quality, quad4_mesh_quality

F64 = torch.float64


def events_us(fn, reps):
    """Mean device time per call of `fn` over `reps` back-to-back calls (after a warm-up), median of 5 such runs."""
    for _ in range(5):
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


def graphed_us(fn, reps, k=16):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(k):
            fn()
    return events_us(g.replay, max(reps // k, 4)) / k


def host_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return sorted(out)[len(out) // 2]


class Clock:
    """Wraps a callable; accumulates its synchronised host time."""

    def __init__(self, fn):
        self.fn, self.total = fn, 0.0

    def __call__(self, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = self.fn(*a, **k)
        torch.cuda.synchronize()
        self.total += time.perf_counter() - t0
        return r


def smooth_field(x):
    """A finite-strain displacement field on [0, 2] x [0, 1] (min det F about 0.5 on these meshes)."""
    return torch.stack([0.15 * torch.sin(2.1 * x[:, 0]) * torch.cos(1.3 * x[:, 1]),
                        0.09 * torch.cos(1.7 * x[:, 0] + 0.3) * torch.sin(2.4 * x[:, 1])], dim=1)


def emit(rec, out):
    line = json.dumps(rec)
    print(line)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main_neo_hookean(a, dev, nx, ny):
    from hidenn_fem_amd.loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    from hidenn_fem_amd.radapt import HyperRAdaptiveSolver, Quad4HyperRAdaptiveSolver, _Mesh, _QuadMesh
    mesher, Solver, Loss, Small = (structured_quad_mesh, Quad4HyperRAdaptiveSolver, Quad4NeoHookeanLoss2D, _QuadMesh) if a.quad \
        else (structured_tri_mesh, HyperRAdaptiveSolver, NeoHookeanLoss2D, _Mesh)
    coords, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
    U = smooth_field(coords)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(U[~bc], "u").to(dev))
    m.u_fixed = U[bc].to(dev)
    lf = Loss(E=2e6, device=dev, dtype=F64)
    down = lambda x: torch.stack([torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], -a.traction)], dim=1)
    ne, nn = m.Nelems, m.Nnodes
    rec = dict(mesh=f"{nx}x{ny} structured {'QUAD4' if a.quad else 'TRI3'}, jitter 0.2", n_elems=ne, n_nodes=nn,
               n_x_rows=int(m.node_coords_free.shape[0]),
               regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)")
    if a.pieces:
        from hidenn_fem_amd.radapt import _HyperMesh, _QuadHyperMesh
        mesh, small = (_QuadHyperMesh if a.quad else _HyperMesh)(m), Small(m)
    else:
        s = Solver(m, lf, t_force=down, max_outer=a.outer, precond=a.precond)
        mesh, small = s.mesh, Small(m)
    j, summary = mesh.deformation()
    rec["state"] = dict(min_J=summary[0].item(), n_inverted=int(summary[1].item()), max_J=j.max().item())
    d = torch.randn(m.node_coords_free.shape, dtype=F64, device=dev) * 1e-3
    alpha = torch.empty((), dtype=F64, device=dev)
    fused_us = graphed_us(lambda: mesh.step_bound(d, 0.25, out=alpha), a.reps)
    alg = 4 * conn.shape[1] * ne + (4 + 4 + 16 + 16 + 16) * nn
    rec["fused_bound"] = dict(us=fused_us, launches=2, alpha=alpha.item(), algorithmic_bytes=alg, tb_per_s=alg / fused_us * 1e-6,
                              note=f"{4 * conn.shape[1]} B/element of connectivity + per node: x_src, u_src 4 B each, x, u, d rows 16 B each")

    # ---- the composition: X + u on the coordinate rows, the small-strain bound on X and on X + u
    u_full = m.u_full.detach()
    xf, xfix = m.node_coords_free.detach(), mesh.fixed()
    u_on_x = u_full[m._idx_free.long()].contiguous()
    yfix = None if xfix is None else (xfix + u_full[m._idx_fixed.long()]).contiguous()
    y = torch.empty_like(xf)
    a2 = torch.empty(2, dtype=F64, device=dev)
    both = torch.empty((), dtype=F64, device=dev)
    from hidenn_fem_amd._lib import ptr

    def composed():
        torch.add(xf, u_on_x, out=y)
        for k, (rows, fixed) in enumerate(((xf, xfix), (y, yfix))):
            small._call("step_bound", ptr(d), 0.25, a2.data_ptr() + 8 * k, rows=(small.x_src, rows, fixed))
        torch.amin(a2, dim=0, out=both)

    composed_us = graphed_us(composed, a.reps)
    rec["composed_bound"] = dict(us=composed_us, launches=6, alpha=both.item(),
                                 note="torch add + 2 x (init + element kernel) + amin; bounds detJ(X) and detJ(X + u) separately")
    rec["fused_over_composed"] = fused_us / composed_us
    rec["measure"] = dict(us=graphed_us(lambda: mesh.deformation(per_element=False), a.reps), launches=3)
    rec["measure_per_element_output"] = dict(us=graphed_us(lambda: mesh.deformation(per_element=True), a.reps))

    # ---- outer iterations from u = 0 under the traction: Newton vs everything else
    if a.outer > 0 and not a.pieces:
        with torch.no_grad():
            m.u_free.zero_()
        m.u_fixed = torch.zeros_like(m.u_fixed)
        m.__dict__.pop("_ufix_cache", None)
        solve_clock = Clock(s.solver.solve)
        s.solver.solve = solve_clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = s.run()
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        rec["outer"] = dict(iterations=info.iterations, reason=info.reason, precond=a.precond, traction=a.traction,
                            newton_iterations=info.newton_iterations, cg_iterations=info.cg_iterations, energy=info.energy,
                            min_J=info.min_J, min_q=info.min_q, alpha=info.alpha, alpha_max=info.alpha_max, trials=info.trials,
                            step_ratio=info.step_ratio, J_step_ratio=info.J_step_ratio, seconds_total=total,
                            seconds_newton=solve_clock.total, seconds_other=total - solve_clock.total,
                            share_outside_newton=(total - solve_clock.total) / total)
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="")
    ap.add_argument("--quad", action="store_true", help="QUAD4 cells (default grid 1415x708: 10^6 cells)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--neo-hookean", action="store_true", help="the finite-strain guard and solver (module docstring)")
    ap.add_argument("--outer", type=int, default=3, help="--neo-hookean: outer iterations to time (0: none)")
    ap.add_argument("--precond", default="amg", help="--neo-hookean: Newton's preconditioner")
    ap.add_argument("--traction", type=float, default=2e4, help="--neo-hookean: the downward traction on the right edge")
    ap.add_argument("--lib", default="", help="the library file to load (default: the tree's own build)")
    ap.add_argument("--pieces", action="store_true", help="the mesh-kernel launches only, no solver")
    a = ap.parse_args()
    if a.lib:
        from hidenn_fem_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda:0")
    nx, ny = (int(v) for v in (a.grid or ("1415x708" if a.quad else "1001x501")).split("x"))
    if a.neo_hookean:
        return main_neo_hookean(a, dev, nx, ny)
    mesher, Solver, quality = (structured_quad_mesh, Quad4RAdaptiveSolver, quad4_mesh_quality) if a.quad else \
        (structured_tri_mesh, RAdaptiveSolver, mesh_quality)
    coords, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
    lf = EnergyLoss2D(device=dev, dtype=F64)
    ne, nn = m.Nelems, m.Nnodes
    rec = dict(mesh=f"{nx}x{ny} structured {'QUAD4' if a.quad else 'TRI3'}, jitter 0.2", n_elems=ne, n_nodes=nn, n_x_rows=int(m.node_coords_free.shape[0]),
               regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)")

    if a.pieces:
        from hidenn_fem_amd.radapt import _Mesh, _QuadMesh
        mesh = (_QuadMesh if a.quad else _Mesh)(m)
    else:
        s = Solver(m, lf, max_outer=3)
        mesh = s.mesh
    d = torch.randn(m.node_coords_free.shape, dtype=F64, device=dev) * 1e-3
    alpha = torch.empty((), dtype=F64, device=dev)
    bound_us = graphed_us(lambda: mesh.step_bound(d, 0.25, out=alpha), a.reps)
    alg = 4 * conn.shape[1] * ne + (4 + 16 + 16) * nn
    rec["step_bound"] = dict(us=bound_us, launches=2, algorithmic_bytes=alg, tb_per_s=alg / bound_us * 1e-6,
                             note=f"{4 * conn.shape[1]} B/element of connectivity + per node: x_src 4 B, x row 16 B, d row 16 B")
    rec["measure"] = dict(us=graphed_us(lambda: mesh.measure(per_element=False), a.reps), launches=3)
    rec["measure_per_element_outputs"] = dict(us=graphed_us(lambda: mesh.measure(per_element=True), a.reps))
    rec["barrier"] = dict(us=graphed_us(lambda: mesh.barrier(1.0), a.reps), launches="2 fills + 1")
    if a.pieces:
        return emit(rec, a.out)
    energy_us = graphed_us(lambda: lf.value_and_grad_(m), a.reps)
    rec["energy_value_and_grad"] = dict(us=energy_us, note="graded energy kernel + tile-energy sum launch")
    rec["step_bound_over_energy"] = bound_us / energy_us
    m.node_coords_free.grad = None
    m.u_free.grad = None

    s.solver.solve()
    x0 = m.node_coords_free.detach().clone()

    def trial():
        with torch.no_grad():
            m.node_coords_free.copy_(x0 + 1e-3 * d)
        return s.objective()

    rec["line_search_trial_host_us"] = host_us(trial, 20)
    with torch.no_grad():
        m.node_coords_free.copy_(x0)
    rec["gradient_host_us"] = host_us(s.objective_and_grad, 20)

    # ---- outer iterations: CG vs everything else
    solve_clock = Clock(s.solver.solve)
    s.solver.solve = solve_clock
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = s.run()
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    rec["outer_T1M"] = dict(iterations=info.iterations, reason=info.reason, cg_iterations=info.cg_iterations,
                            energy=info.energy, alpha=info.alpha, alpha_max=info.alpha_max, trials=info.trials,
                            min_q=info.min_q, seconds_total=total, seconds_cg=solve_clock.total,
                            seconds_other=total - solve_clock.total,
                            other_over_cg=(total - solve_clock.total) / solve_clock.total)

    # ---- the example-4 plate (36 k elements)
    sides = {"up": 0, "down": 0, "right": 2, "left": 1}
    if a.quad:
        nodes, conn4, geom4, bc4, mn4, edges4 = structured_quad_mesh(200, 100, length=2.0, height=1.0, boundaries=sides)
    else:
        nodes, conn4, geom4, bc4, mn4, edges4 = generate_mesh(2.0, 1.0, [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)],
                                                              sides, 200, 100)
    for key, w in (("example4_plate", 0.0), ("example4_plate_barrier_0.05", 0.05)):
        torch.manual_seed(0)
        p = PiecewiseLinearShapeNN2D(nodes.double(), conn4, boundary_mask=geom4, dirichlet_mask=bc4, u_fixed=0.0,
                                     neumann_edges=edges4).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pi = Solver(p, lf, max_outer=50, quality_weight=w).run()
        torch.cuda.synchronize()
        mq = quality(p)
        rec[key] = dict(n_elems=p.Nelems, quality_weight=w, iterations=pi.iterations, reason=pi.reason,
                        energy_frozen=pi.energy[0], energy_final=pi.energy[-1], decrease=pi.energy[0] - pi.energy[-1],
                        cg_iterations=pi.cg_iterations, min_q_initial=pi.min_q[0], min_q_final=mq.min_q,
                        n_inverted=mq.n_inverted, seconds=time.perf_counter() - t0, energy=pi.energy)
    emit(rec, a.out)


if __name__ == "__main__":
    main()
