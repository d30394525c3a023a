#!/usr/bin/env python3
"""J2 elastoplastic kernels and one load step at T1M (dev tool; gates nothing): the 10^6-element TRI3 benchmark mesh
(1001 x 501 nodes), left edge clamped, a vertical traction on the right edge, fp64 (hidenn_fem_amd/plasticity.py,
csrc/tri3_j2.hip).

One JSON object -> `profiles/plasticity/plasticity_timing_T1M.json`:
  * `launches`: the update launch (with and without the state write-out), the linearisation launch and the J2 tangent apply,
    against the two baselines ON THE SAME PLAN IN THE SAME RUN: the Neo-Hookean tangent apply and the Neo-Hookean energy launch.
    The one stated expectation: the J2 apply is no slower than the Neo-Hookean tangent apply (it drops one gathered row array
    and all transcendental and state arithmetic, and adds 40 bytes per slot of coalesced records);
  * `step`: one load step into the plastic range with AMG and with block Jacobi: wall time, Newton and CG iterations, plastic
    fraction.
Launch times: hipGraph replay of `--reps` back-to-back launches on preallocated buffers between device events, median of
`--samples` replays after two warm-up replays.  A run that was not made is recorded as "not measured yet".

    python scripts/plasticity_timing.py [--reps 20] [--samples 7] [--out-dir profiles/plasticity] [--small] [--no-step]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.loss import NeoHookeanLoss2D
from hidenn_fem_amd.mesh import structured_tri_mesh
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
from hidenn_fem_amd.newton import NewtonKrylovSolver
from hidenn_fem_amd.plasticity import ElastoplasticSolver, J2PlasticityLoss2D

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


def traction(x):
    return torch.stack([torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], 1e4)], dim=1)


def measure(nx, ny, reps, samples, with_step):
    dev = torch.device("cuda:0")
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)

    def model():
        m = PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
        with torch.no_grad():
            m.u_free.zero_()
        return m

    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    lf = J2PlasticityLoss2D(sigma_y=6e4, hardening=5e8, gauss_order=1, device=dev, dtype=F64)
    m = model()
    s = ElastoplasticSolver(m, lf, t_force=traction, precond="block_jacobi", rtol=1e-8)
    n = s.n_u
    gen = torch.Generator(device=dev).manual_seed(0)
    # a state with both branches: a random field of about the yield strain over one element
    with torch.no_grad():
        m.u_free.copy_(torch.randn((n, 2), dtype=F64, device=dev, generator=gen) * (1e-5 * 2.0 / nx))
    out, _ = s.evaluate()
    frac = out[1].item() / s.ne
    P, Q = torch.randn((n, 2), dtype=F64, device=dev, generator=gen), torch.empty((n, 2), dtype=F64, device=dev)
    pq = torch.empty((), dtype=F64, device=dev)
    res = dict(mesh=dict(nodes=int(nc.shape[0]), elements=int(conn.shape[0]), tiles=s.plan.n_tiles, record_doubles=int(s._tan.numel())),
               plastic_fraction_of_the_timed_state=frac, reps=reps, samples=samples)
    launches = {}

    def upd(write):
        s._write = write
        return lambda: s._energy(s._u, s._g)
    launches["j2_update_us"], _ = graph_us(upd(0), reps, samples)
    launches["j2_update_with_state_write_us"], _ = graph_us(upd(1), reps, samples)
    s._write = 0
    launches["j2_linearise_us"], _ = graph_us(s._linearise, reps, samples)
    apply_j2 = lambda: _lib.check(L.hfem_cg_apply(s._h, p(P), p(Q), p(pq), st))
    launches["j2_apply_us"], launches["j2_apply_samples_us"] = graph_us(apply_j2, reps, samples)
    # ---- the baselines on the same plan: the Neo-Hookean tangent apply and energy launch at the same displacement field
    nh = NeoHookeanLoss2D(device=dev, dtype=F64, plane="strain")
    sn = NewtonKrylovSolver(m, nh, t_force=traction, precond="block_jacobi")
    assert sn.plan is s.plan
    sn.apply(P)
    apply_nh = lambda: _lib.check(L.hfem_cg_apply(sn._h, p(P), p(Q), p(pq), st))
    launches["neo_hookean_apply_us"], launches["neo_hookean_apply_samples_us"] = graph_us(apply_nh, reps, samples)
    launches["neo_hookean_energy_us"], _ = graph_us(lambda: sn._energy(sn._u, sn._g), reps, samples)
    launches["neo_hookean_linearise_us"], _ = graph_us(sn._linearise, reps, samples)
    launches["j2_apply_over_neo_hookean_apply"] = launches["j2_apply_us"] / launches["neo_hookean_apply_us"]
    res["launches"] = launches
    print(json.dumps(launches))
    res["step"] = "not measured yet"
    if with_step:
        steps = {}
        for precond in ("amg", "block_jacobi"):
            mm = model()
            ss = ElastoplasticSolver(mm, lf, t_force=traction, precond=precond, rtol=1e-8)
            ss.refresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = ss.solve(0.5)
            torch.cuda.synchronize()
            steps[precond] = dict(wall_s=time.perf_counter() - t0, newton=info.newton_iterations, cg=info.cg_iterations,
                                  reason=info.reason, plastic_fraction=ss.plastic_fraction)
            print(precond, json.dumps(steps[precond]))
        res["step"] = steps
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out-dir", default="profiles/plasticity")
    ap.add_argument("--small", action="store_true", help="a 101 x 51 mesh: a smoke run of this script, not a measurement")
    ap.add_argument("--no-step", action="store_true", help="the launches only")
    a = ap.parse_args()
    nx, ny = (101, 51) if a.small else (1001, 501)
    r = measure(nx, ny, a.reps, a.samples, not a.no_step)
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "plasticity_timing_%s.json" % ("small" if a.small else "T1M"))
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    print("wrote", path)
