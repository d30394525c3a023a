#!/usr/bin/env python3
"""Element-scaled stiffness and SIMP topology optimisation at T1M / Q1M (dev tool; gates nothing): the 10^6-element TRI3
(1001 x 501 nodes) and, with `--quad`, QUAD4 (1415 x 708 nodes) benchmark meshes, left edge clamped, fp64, physical convention
(hidenn_fem_amd/topopt.py, csrc/topopt.hip).

One JSON object -> `profiles/topopt/topopt_timing_{T1M,Q1M}.json`:
  * `apply`: the scaled apply q = K(w) p against the plain apply q = K p of the same tree on the same plan.  The one stated
    expectation: the scaled apply moves one more 8-byte word per element than the plain one (`extra_bytes_per_launch`);
  * `launches`: the weights launch, the energy and sensitivity launch, the filter launch, one bisection step (the slope between
    OC updates of 1 and 21 halvings) and one whole OC update (60 halvings);
  * `amg_setup`: the numeric AMG setup on K(w) against the plain one (wall, device-synchronised, median);
  * `design`: 25 design iterations end to end with AMG: wall per iteration and the PCG iterations at 1, 10 and 25, per `e_min`
    of `--e-mins` (the AMG iteration count at a contrast of 1e-9 is this feature's open question).
Launch times: hipGraph replay of `--reps` back-to-back launches on preallocated buffers between device events, median of
`--samples` replays after two warm-up replays.

    python scripts/topopt_timing.py [--quad] [--reps 20] [--samples 7] [--e-mins 1e-9,1e-6,1e-3] [--out-dir profiles/topopt] [--small]
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
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
from hidenn_fem_amd.topopt import TopologyOptimizer

F64 = torch.float64


def median(xs):
    return sorted(xs)[len(xs) // 2]


def graph_us(fn, reps, samples):
    """Median device time per call of `fn`: `reps` calls captured in one graph, `samples` timed replays after two warm-ups."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    out = []
    for k in range(samples + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            out.append(a.elapsed_time(b) * 1e3 / reps)
    return median(out), out


def measure(name, quad, nx, ny, reps, samples, e_mins, n_design, max_iter):
    dev = torch.device("cuda:0")
    mesher, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)

    def model():
        m = cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
        with torch.no_grad():
            m.u_free.zero_()
        return m

    lf = EnergyLoss2D(device=dev, dtype=F64, grad_convention="physical")
    L, p = _lib.lib(), _lib.ptr
    m = model()
    t0 = time.perf_counter()
    opt = TopologyOptimizer(m, lf, 0.4, precond="amg", rtol=1e-8)
    create_s = time.perf_counter() - t0
    s, ew, ne = opt.solver, opt.weights, opt.ne
    n = s.n_u
    g = torch.Generator(device=dev).manual_seed(0)
    P, Q = torch.randn((n, 2), dtype=F64, device=dev, generator=g), torch.empty((n, 2), dtype=F64, device=dev)
    pq = torch.empty((), dtype=F64, device=dev)
    apply_fn = lambda: _lib.check(L.hfem_cg_apply(s._h, p(P), p(Q), p(pq), _lib.stream_ptr(dev)))
    # ---- apply: plain, then scaled, one solver, one plan
    s._scale = None
    s.refresh()
    t_plain, s_plain = graph_us(apply_fn, reps, samples)
    rho = (0.05 + 0.95 * torch.rand(ne, dtype=F64, device=dev, generator=g)).contiguous()
    ew.simp(rho, 3.0, 1e-9)
    s._scale = ew
    s.refresh()
    t_scaled, s_scaled = graph_us(apply_fn, reps, samples)
    slots = ew.w_slot.numel()
    apply = dict(plain_us=t_plain, scaled_us=t_scaled, scaled_over_plain=t_scaled / t_plain, plain_samples_us=s_plain,
                 scaled_samples_us=s_scaled, extra_bytes_per_launch=8 * slots, extra_bytes_per_element=8 * slots / ne,
                 extra_us_at_the_measured_difference=t_scaled - t_plain,
                 extra_gbytes_per_s=8 * slots / max(t_scaled - t_plain, 1e-9) * 1e-3, tile=dict(s.plan.stats))
    # ---- the small launches
    ce, dc = torch.empty(ne, dtype=F64, device=dev), torch.empty(ne, dtype=F64, device=dev)
    out = torch.empty(ne, dtype=F64, device=dev)
    mat = s._tables[0]
    t_w, _ = graph_us(lambda: ew.simp(rho, 3.0, 1e-9), reps, samples)
    t_e, _ = graph_us(lambda: ew.energy(s._xf, s._xfix, P, mat, lf._W, s.phys, rho, 3.0, 1e-9, ce, dc), reps, samples)
    t_f, _ = graph_us(lambda: _lib.check(L.hfem_topt_filter(ew._h, p(rho), p(out), 0, _lib.stream_ptr(dev))), reps, samples)
    t_ft, _ = graph_us(lambda: _lib.check(L.hfem_topt_filter(ew._h, p(rho), p(out), 1, _lib.stream_ptr(dev))), reps, samples)
    dcf = -(torch.rand(ne, dtype=F64, device=dev, generator=g) + 1e-3)
    rn, rf = torch.empty(ne, dtype=F64, device=dev), torch.empty(ne, dtype=F64, device=dev)
    target = 0.6 * float(opt.volumes.sum())                  # the random design (mean 0.52) is feasible: every step halves
    oc = lambda nb: (lambda: ew.oc(rho, dcf, opt._dv, target, 0.2, nb, rn, rf))
    t_oc1, _ = graph_us(oc(1), 4, samples)
    t_oc21, _ = graph_us(oc(21), 4, samples)
    t_oc60, _ = graph_us(oc(60), 2, samples)
    st = ew.status()
    launches = dict(weights_us=t_w, energy_us=t_e, filter_us=t_f, filter_transpose_us=t_ft, oc_bisection_step_us=(t_oc21 - t_oc1) / 20,
                    oc_update_60_us=t_oc60, oc_steps_of_the_last_update=st["steps"],
                    filter_radius=opt.filter_radius, handle_create_s=create_s)
    # ---- numeric AMG setup, plain against scaled
    plain_s, scaled_s = [], []
    for _ in range(samples):
        s._amg.setup(s._xf, s._xfix, mat, float(lf._W))
        plain_s.append(s._amg.seconds)
        s._amg.setup_scaled(s._xf, s._xfix, mat, float(lf._W), ew.w_elem)
        scaled_s.append(s._amg.seconds)
    amg_setup = dict(plain_ms=1e3 * median(plain_s), scaled_ms=1e3 * median(scaled_s), plain_samples_ms=[1e3 * v for v in plain_s],
                     scaled_samples_ms=[1e3 * v for v in scaled_s], hierarchy=s._amg.report())
    del opt, s, ew
    # ---- design iterations end to end
    design = {}
    for e_min in e_mins:
        o = TopologyOptimizer(model(), lf, 0.4, e_min=e_min, precond="amg", rtol=1e-8, max_iter=max_iter)
        rows = []
        for k in range(n_design):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = o.step()
            torch.cuda.synchronize()
            rows.append(dict(iteration=k + 1, wall_ms=1e3 * (time.perf_counter() - t0), pcg_iterations=info.iterations,
                             converged=info.converged, compliance=info.compliance, change=info.change, feasible=info.feasible))
        pick = [r for r in rows if r["iteration"] in (1, 10, 25)]
        design[f"{e_min:g}"] = dict(pcg_iterations_at_1_10_25=[r["pcg_iterations"] for r in pick],
                                    wall_ms_at_1_10_25=[r["wall_ms"] for r in pick],
                                    median_wall_ms=median([r["wall_ms"] for r in rows[1:]] or [rows[0]["wall_ms"]]), iterations=rows)
        del o
    return dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2, left edge clamped",
                n_elems=ne, free_dofs=2 * n, penal=3.0, volume_fraction=0.4,
                timing=f"hipGraph replay of {reps} launches between device events, median of {samples} replays after 2 warm-ups",
                apply=apply, launches=launches, amg_setup=amg_setup, design=design,
                design_note=f"rtol 1e-8, max_iter {max_iter}, warm start, wall per step() with its host synchronisations (status reads, the coarse "
                            "inverse of the AMG setup) and, at iteration 1, the graph capture")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--e-mins", default="1e-9,1e-6,1e-3")
    ap.add_argument("--design-iterations", type=int, default=25)
    ap.add_argument("--max-iter", type=int, default=2000, help="PCG iteration cap of a design iteration's solve")
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--quad", action="store_true", help="Q1M instead of T1M")
    ap.add_argument("--small", action="store_true", help="101x51 / 142x71 nodes (a check that the script runs)")
    a = ap.parse_args()
    name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
    if a.small:
        nx, ny = nx // 10 + 1, ny // 10 + 1
    line = json.dumps(measure(name, quad, nx, ny, a.reps, a.samples, [float(v) for v in a.e_mins.split(",") if v],
                              a.design_iterations, a.max_iter))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"topopt_timing_{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
