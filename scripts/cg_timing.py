#!/usr/bin/env python3
"""Frozen-mesh CG solve at T1M (dev tool): 10^6 TRI3, fp64, default traction (hidenn_fem_amd/solve.py, csrc/cg.hip,
csrc/tri3_cg.hip).

Records, as one JSON object:
  * the standalone apply launch (q = K p) and its fraction of 8 TB/s on the algorithmic bytes 12 Ne + 48 Nn (slot records,
    coordinate and p rows read, q rows written -- the fused p-update's z / p_old reads and p store are not counted here);
  * the graded energy evaluation on the same mesh (value_and_grad_: the pair kernel + its tile-energy sum);
  * one CG iteration (apply + vector update) under graph replay, iters_per_graph = 16;
  * iterations and wall time to rtol 1e-8 with both preconditioners (host clock around solve(), synchronised);
  * the A/B: a torch-composed PCG whose matvec is value_and_grad_(p) - value_and_grad_(0), same block-Jacobi blocks.
Times are device events around back-to-back graph replays of the same buffers (launch times: 16 launches per graph; the
eager ctypes / Python numbers beside them are host-bound): the per-iteration working set (~120 MB) stays in
the 256 MB Infinity Cache, so these are cache-regime numbers.

    python scripts/cg_timing.py [--grid 1001x501] [--reps 200] [--out profiles/cg/cg_timing_T1M.json]

``--quad``: the same record for Q1M, 10^6 QUAD4 cells on the 1001 x 1001 grid (Quad4FrozenMeshSolver, csrc/quad4_cg.hip; the
algorithmic bytes are 16 Ne + 48 Nn: two record words per cell):

    python scripts/cg_timing.py --quad [--out profiles/cg/cg_timing_Q1M.json]
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
from hidenn_fem_amd.loss import EnergyLoss2D
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver

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
    """Device time per call of `fn` with the host out of the way: k calls captured in one graph, replayed back to back."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(k):
            fn()
    return events_us(g.replay, max(reps // k, 4)) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="")
    ap.add_argument("--quad", action="store_true", help="QUAD4 cells (default grid 1001x1001) instead of TRI3 (1001x501)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nx, ny = (int(v) for v in (a.grid or ("1001x1001" if a.quad else "1001x501")).split("x"))
    Solver = Quad4FrozenMeshSolver if a.quad else FrozenMeshSolver
    if a.quad:
        coords, conn, geom, bc, mn, edges = structured_quad_mesh(nx, ny, length=2.0, height=2.0, jitter=0.2, seed=0, dtype=F64)
    else:
        coords, conn, geom, bc, mn, edges = structured_tri_mesh(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
    lf = EnergyLoss2D(device=dev, dtype=F64)
    ne, nn = m.Nelems, m.Nnodes
    rec = dict(mesh=f"{nx}x{ny} structured {'QUAD4' if a.quad else 'TRI3'}, jitter 0.2", n_elems=ne, n_nodes=nn, n_u_rows=int(m.u_free.shape[0]),
               plan=dict((k, v) for k, v in m.tile_plan().stats.items() if k in ("n_tiles", "threads_per_tile", "paired",
                                                                                   "max_tile_nodes", "max_tile_owned")),
               regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)")
    u_init = m.u_free.detach().clone()

    # ---- apply vs the graded energy launch
    s = Solver(m, lf, rtol=1e-8)
    s.refresh()
    p = torch.randn(m.u_free.shape, dtype=F64, device=dev) * 1e-4
    q, pq = torch.empty_like(p), torch.empty((), dtype=F64, device=dev)
    L = _lib.lib()
    apply_one = lambda: L.hfem_cg_apply(s._h, p.data_ptr(), q.data_ptr(), pq.data_ptr(), _lib.stream_ptr(dev))
    apply_host_us = events_us(apply_one, a.reps)
    apply_us = graphed_us(apply_one, a.reps)
    alg_bytes = (16 if a.quad else 12) * ne + 48 * nn
    rec["apply"] = dict(us=apply_us, algorithmic_bytes=alg_bytes, tb_per_s=alg_bytes / apply_us * 1e-6,
                        fraction_of_8TBps=alg_bytes / apply_us * 1e-6 / 8.0, us_eager_ctypes=apply_host_us)
    energy_us = graphed_us(lambda: lf.value_and_grad_(m), a.reps)
    rec["energy_value_and_grad"] = dict(us=energy_us, us_eager=events_us(lambda: lf.value_and_grad_(m), a.reps),
                                        note="graded energy kernel + tile-energy sum launch")
    rec["ratio_apply_over_energy"] = apply_us / energy_us
    rec["bar_apply_faster_than_energy"] = apply_us < energy_us

    # ---- one captured iteration (rtol = 0: never halts while timed)
    s0 = Solver(m, lf, rtol=0.0, atol=0.0, max_iter=10 ** 9, iters_per_graph=16)
    s0.refresh()
    with torch.no_grad():
        s0._u.copy_(u_init)
        s0._gradient(s0._u, s0._g0)
        s0._gradient(s0._zero, s0._gz)
    s0._start(0.0, 0.0, 10 ** 9)
    it_us = events_us(s0._replay, max(a.reps // 16, 4)) / 16
    rec["iteration_graphed"] = dict(us=it_us, iters_per_graph=16, launches_per_iteration=2)

    # ---- to rtol 1e-8, both preconditioners
    rec["solve_rtol_1e-8"] = {}
    for pc in ("block_jacobi", "none"):
        with torch.no_grad():
            m.u_free.copy_(u_init)
        sv = Solver(m, lf, precond=pc, rtol=1e-8)
        sv.refresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = sv.solve()
        torch.cuda.synchronize()
        rec["solve_rtol_1e-8"][pc] = dict(iterations=info.iterations, seconds=time.perf_counter() - t0, reason=info.reason,
                                          residual_over_rhs=info.residual_norm / info.rhs_norm)

    # ---- A/B: torch-composed PCG, matvec = value_and_grad_(p) - value_and_grad_(0)
    with torch.no_grad():
        m.u_free.zero_()
    lf.value_and_grad_(m)
    g_zero = m.u_free.grad.clone()
    d = s.diag
    det = d[:, 0] * d[:, 2] - d[:, 1] ** 2
    dinv = torch.stack([d[:, 2] / det, -d[:, 1] / det, d[:, 0] / det], dim=1)

    def prec(r):
        return torch.stack([dinv[:, 0] * r[:, 0] + dinv[:, 1] * r[:, 1], dinv[:, 1] * r[:, 0] + dinv[:, 2] * r[:, 1]], dim=1)

    def matvec(v):
        with torch.no_grad():
            m.u_free.copy_(v)
        lf.value_and_grad_(m)
        return m.u_free.grad - g_zero

    with torch.no_grad():
        u = u_init.clone()
        m.u_free.copy_(u)
        lf.value_and_grad_(m)
        r = -m.u_free.grad.clone()
        z = prec(r)
        pp = z.clone()
        rho = (r * z).sum()
        state = [u, r, z, pp, rho]

        def torch_iter():
            u, r, z, pp, rho = state
            qq = matvec(pp)
            alpha = rho / (pp * qq).sum()
            u.add_(alpha * pp)
            r.sub_(alpha * qq)
            z = prec(r)
            rho_new = (r * z).sum()
            pp.mul_(rho_new / rho).add_(z)
            state[:] = [u, r, z, pp, rho_new]
        torch_us = events_us(torch_iter, max(a.reps // 4, 10))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(16):
                torch_iter()
        torch_graph_us = events_us(g.replay, max(a.reps // 16, 4)) / 16
    rec["torch_composed_pcg"] = dict(us_eager=torch_us, us_graphed=torch_graph_us)
    rec["ratio_captured_over_torch_graphed"] = it_us / torch_graph_us
    rec["ratio_captured_over_torch_eager"] = it_us / torch_us
    rec["bar_iteration_at_most_half_of_torch"] = it_us <= 0.5 * torch_graph_us
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
