#!/usr/bin/env python3
"""The Neo-Hookean launch against the linear physical-convention launch on the SAME tile plan, at T1M (dev tool; gates
nothing): 1001 x 501 nodes, 10^6 TRI3, fp64, jitter 0.2, on the mesh's one-element-per-slot plan (plan_elem_order 3).

  * `neo_hookean`: hfem_tri3_hyper_energy_plan (tile kernel + one-block finish), both gradients;
  * `linear_physical`: hfem_tri3_energy_plan with HFEM_FLAG_PHYSICAL_GRAD on that plan -- the general physical instance of
    the register-prefetched kernel (512 threads, two node and four slot records per thread, write-through stores);
  * device events around back-to-back calls on preallocated buffers, the two ALTERNATING in one process, median of 7 windows
    each (every window a few thousand launches);
  * the algorithmic bytes (every array read or written once: parameter rows in, gradient rows out, the plan's row maps, slot
    records and descriptors) -- the same for both -- and the time they take at 8 TB/s.
Cache regime: the working set stays in the 256 MB Infinity Cache (same buffers every launch).

``--quad``: the same record at Q1M -- 1001 x 1001 nodes, 10^6 QUAD4 cells on [0, 2]^2, fp64, jitter 0.2, on the model's own
QUAD4 plan: hfem_quad4_hyper_energy_plan against hfem_quad4_energy_plan_ex with HFEM_FLAG_PHYSICAL_GRAD on the same plan and
buffers (256 threads per tile; slot records are two words).  Written to hyper_timing_Q1M.json.

    python scripts/hyper_timing.py [--quad] [--reps 3000] [--out-dir profiles/hyper] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D, HFEM_FLAG_NO_EDGES, HFEM_FLAG_PHYSICAL_GRAD
from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
from hidenn_fem_amd.plan import model_plan

F64 = torch.float64
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def field(x):
    return torch.stack([0.25 * torch.sin(2.1 * x[:, 0]) * torch.cos(1.3 * x[:, 1]),
                        0.15 * torch.cos(1.7 * x[:, 0] + 0.3) * torch.sin(2.4 * x[:, 1])], dim=1)


def measure(nx, ny, reps):
    dev = torch.device("cuda:0")
    coords, conn, *_ = structured_tri_mesh(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    m = PiecewiseLinearShapeNN2D(coords, conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(field(coords), "u"))
    m = m.to(dev)
    plan = model_plan(m, 0, paired=False)
    nh = NeoHookeanLoss2D(device=dev, dtype=F64)
    lin = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    x, u = m.node_coords_free.detach(), m.u_free.detach()
    gx, gu = torch.empty_like(x), torch.empty_like(u)
    loss, info = torch.zeros((), dtype=F64, device=dev), torch.zeros(2, dtype=F64, device=dev)
    work = torch.empty(3 * plan.n_tiles, dtype=F64, device=dev)
    L, st, p = _lib.lib(), _lib.stream_ptr(dev), _lib.ptr
    lame, mat, tc = (C.c_double * 2)(*nh.lame), (C.c_double * 4)(*lin._mat), (C.c_double * 4)(0, 0, 0, 0)

    def neo():
        _lib.check(L.hfem_tri3_hyper_energy_plan(plan.handle, 0, p(x), None, p(u), None, lame, nh._W, None, None, tc, p(loss), p(info),
                                                 p(work), p(gx), p(gu), HFEM_FLAG_NO_EDGES, st), "hfem_tri3_hyper_energy_plan")

    def linear():
        _lib.check(L.hfem_tri3_energy_plan(plan.handle, p(x), None, p(u), None, mat, lin._W, None, None, tc, 0, -1, p(loss), p(gx),
                                           p(gu), HFEM_FLAG_NO_EDGES | HFEM_FLAG_PHYSICAL_GRAD, st), "hfem_tri3_energy_plan")

    for _ in range(20):
        neo()
        linear()
    torch.cuda.synchronize()
    neo()
    nh_loss, min_j = loss.item(), info[0].item()
    t = {"neo": [], "lin": []}
    for _ in range(7):                                             # alternating windows
        t["neo"].append(window_us(neo, reps))
        t["lin"].append(window_us(linear, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    s = plan.stats
    nbytes = 64 * m.Nnodes + 8 * s["tile_node_total"] + 4 * s["tile_elem_total"] + 32 * s["n_tiles"]
    bound = nbytes / HBM_BYTES_PER_US
    return dict(mesh=f"T1M: {nx}x{ny} structured TRI3, jitter 0.2", n_elems=m.Nelems, n_nodes=m.Nnodes,
                plan=dict(elem_order=3, paired=bool(s["paired"]), n_tiles=s["n_tiles"], max_tile_nodes=s["max_tile_nodes"],
                          max_tile_elems=s["max_tile_elems"], threads_per_tile=512),
                regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)",
                reps_per_window=reps, windows=7, energy=nh_loss, min_J=min_j,
                algorithmic_bytes=nbytes, us_at_8TBps=bound,
                neo_hookean=dict(us=med["neo"], launches=2, windows_us=t["neo"], times_the_byte_bound=med["neo"] / bound),
                linear_physical=dict(us=med["lin"], launches=2, windows_us=t["lin"], times_the_byte_bound=med["lin"] / bound),
                ratio_neo_over_linear=med["neo"] / med["lin"])


def measure_quad(nx, ny, reps):
    dev = torch.device("cuda:0")
    coords, conn, *_ = structured_quad_mesh(nx, ny, length=2.0, height=2.0, jitter=0.2, seed=0, dtype=F64)
    m = PiecewiseLinearShapeNN2D(coords, conn)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(field(coords), "u"))
    m = m.to(dev)
    plan = m.tile_plan(0)
    nh = Quad4NeoHookeanLoss2D(device=dev, dtype=F64)
    lin = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    x, u = m.node_coords_free.detach(), m.u_free.detach()
    gx, gu = torch.empty_like(x), torch.empty_like(u)
    loss, info = torch.zeros((), dtype=F64, device=dev), torch.zeros(2, dtype=F64, device=dev)
    work = torch.empty(3 * plan.n_tiles, dtype=F64, device=dev)
    L, st, p = _lib.lib(), _lib.stream_ptr(dev), _lib.ptr
    lame, mat, tc = (C.c_double * 2)(*nh.lame), (C.c_double * 4)(*lin._mat), (C.c_double * 4)(0, 0, 0, 0)

    def neo():
        _lib.check(L.hfem_quad4_hyper_energy_plan(plan.handle, 0, p(x), None, p(u), None, lame, None, None, tc, p(loss), p(info),
                                                  p(work), p(gx), p(gu), HFEM_FLAG_NO_EDGES, st), "hfem_quad4_hyper_energy_plan")

    def linear():
        _lib.check(L.hfem_quad4_energy_plan_ex(plan.handle, 0, p(x), None, p(u), None, mat, None, None, tc, 0, -1, p(loss), p(gx),
                                               p(gu), HFEM_FLAG_NO_EDGES | HFEM_FLAG_PHYSICAL_GRAD, st), "hfem_quad4_energy_plan_ex")

    for _ in range(20):
        neo()
        linear()
    torch.cuda.synchronize()
    neo()
    torch.cuda.synchronize()
    nh_loss, min_j, n_inv = loss.item(), info[0].item(), info[1].item()
    t = {"neo": [], "lin": []}
    for _ in range(7):                                             # alternating windows
        t["neo"].append(window_us(neo, reps))
        t["lin"].append(window_us(linear, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    s = plan.stats
    nbytes = 64 * m.Nnodes + 8 * s["tile_node_total"] + 8 * s["tile_elem_total"] + 32 * s["n_tiles"]
    bound = nbytes / HBM_BYTES_PER_US
    return dict(mesh=f"Q1M: {nx}x{ny} structured QUAD4, jitter 0.2", n_elems=m.Nelems, n_nodes=m.Nnodes,
                plan=dict(n_tiles=s["n_tiles"], max_tile_nodes=s["max_tile_nodes"], max_tile_owned=s["max_tile_owned"],
                          max_tile_elems=s["max_tile_elems"], threads_per_tile=256),
                regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)",
                reps_per_window=reps, windows=7, energy=nh_loss, min_J=min_j, inverted=n_inv,
                algorithmic_bytes=nbytes, us_at_8TBps=bound,
                neo_hookean=dict(us=med["neo"], launches=2, windows_us=t["neo"], times_the_byte_bound=med["neo"] / bound),
                linear_physical=dict(us=med["lin"], launches=2, windows_us=t["lin"], times_the_byte_bound=med["lin"] / bound),
                ratio_neo_over_linear=med["neo"] / med["lin"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3000)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--small", action="store_true", help="101x51 nodes (a check that the script runs)")
    ap.add_argument("--quad", action="store_true", help="Q1M: the QUAD4 launch against the linear QUAD4 launch")
    a = ap.parse_args()
    if a.quad:
        nx, ny = (101, 101) if a.small else (1001, 1001)
        line = json.dumps(measure_quad(nx, ny, a.reps))
    else:
        nx, ny = (101, 51) if a.small else (1001, 501)
        line = json.dumps(measure(nx, ny, a.reps))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, ("hyper_timing_Q1M.json" if a.quad else "hyper_timing_T1M.json") if not a.small else "hyper_timing_small.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
