#!/usr/bin/env python3
"""Finite-strain dynamics at T1M / Q1M (dev tool; gates nothing): the 10^6-element TRI3 (1001 x 501 nodes) and, with `--quad`,
QUAD4 (1415 x 708 nodes) benchmark meshes, left edge clamped, fp64, E = 2e6, rho = 2, consistent mass
(hidenn_fem_amd/dynamics.py HyperNewmarkSolver, the MASS instances of csrc/tri3_hyper_cg.hip and csrc/quad4_hyper_cg.hip,
csrc/dynamics.hip).

One JSON object -> `profiles/dynamics/hyper_dynamics_timing_{T1M,Q1M}.json`:
  * `apply`: the shifted tangent apply q = (c_K K_T + c_M M) p against the plain tangent apply q = K_T p on the same plan, the
    same linearisation point and the same build, in groups of five windows (plain, shifted, plain: the handle holds one binding at
    a time and is rebound between the groups, outside the events), the window means of each (their spread
    is the run-to-run spread a comparison has to respect) and the ratio of the medians; the one-column `hfem_mass_apply` and
    the composition "plain + mass" for comparison.  The linearisation point is 0.1 x the test field of
    tests/hyper_reference.py (strains of a few %).
  * `vector`: the two Newton vector kernels with their algorithmic bytes and the time those take at 8 TB/s;
  * `steps`: Newton and CG iterations, min J and wall time per step over `--steps` steps at dt = T1 / 20 and T1 / 400 for
    `amg` and `block_jacobi` (rtol 1e-10); T1 of the linearised pencil from `ModalSolver` (one mode).  The load is a downward
    dead traction on the right edge, raised smoothly, load(t) = (1 - cos(2 pi t / T1)) / 2: a step load puts its whole first
    acceleration into the loaded edge's nodes, which at dt = T1/20 on a 10^6-element mesh moves them by many element sizes.
Launch times: device events around back-to-back launches on preallocated buffers, median of 5 windows.  Cache regime: the same
buffers every call; a vector is 8 MB at T1M, so the vector kernels' working set (48-56 MB) sits in the 256 MB Infinity Cache,
as do the apply's rows.

`--plain-only --lib PATH` times the plain tangent apply alone on another build of the library (the parent commit's), the check
that the MASS = false instances did not slow down.

    python scripts/hyper_dynamics_timing.py [--quad] [--reps 20] [--steps 3] [--out-dir profiles/dynamics] [--small]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from dynamics_timing import entry, median
from hidenn_fem_amd import _lib

F64 = torch.float64
RHO, E_SOFT, TRACTION = 2.0, 2e6, 500.0
NEW_SYMBOLS = ("hfem_cg_setup_hyper_shifted", "hfem_newmark_trial", "hfem_newmark_residual")


def windows_us(fns, reps):
    """Mean device time per call over `reps` back-to-back calls, five windows per callable, the callables' windows alternating
    (a, b, a, b, ...) so that all see the same clock regime.  -> one sorted list of five per callable"""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(5):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / reps)
    return [sorted(o) for o in out]


def field(x):
    """0.1 x the finite-strain test field of tests/hyper_reference.py: strains of a few %, no element near inversion."""
    return 0.1 * torch.stack([0.25 * torch.sin(2.1 * x[:, 0]) * torch.cos(1.3 * x[:, 1]),
                              0.15 * torch.cos(1.7 * x[:, 0] + 0.3) * torch.sin(2.4 * x[:, 1])], dim=1)


def measure(name, quad, nx, ny, reps, n_steps, plain_only):
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    from hidenn_fem_amd.newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver
    dev = torch.device("cuda:0")
    mesher, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = mesher(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)

    def model(u=None):
        m = cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
        with torch.no_grad():
            m.u_free.zero_()
            if u is not None:
                m.u_free.copy_(m.from_caller_order(u[~bc], "u"))
        return m

    lf = (Quad4NeoHookeanLoss2D if quad else NeoHookeanLoss2D)(E=E_SOFT, device=dev, dtype=F64)
    m = model(field(nc))
    head = dict(mesh=f"{name}: {nx}x{ny} structured {'QUAD4' if quad else 'TRI3'}, jitter 0.2, left edge clamped",
                n_elems=m.Nelems, n_nodes=m.Nnodes, density=RHO, E=E_SOFT, mass="consistent",
                timing="device events around back-to-back launches on preallocated buffers, five windows, median")
    g = torch.Generator(device=dev).manual_seed(0)
    if plain_only:
        nw = (Quad4NewtonKrylovSolver if quad else NewtonKrylovSolver)(m, lf)
        p = torch.randn((nw.n_u, 2), dtype=F64, device=dev, generator=g)
        q, pq = nw.apply(p)                                  # refresh + linearise
        call = lambda: _lib.check(_lib.lib().hfem_cg_apply(nw._h, p.data_ptr(), q.data_ptr(), pq.data_ptr(), _lib.stream_ptr(dev)))
        w, = windows_us([call], reps)
        return dict(head, library=os.path.basename(_lib.LIB_PATH), apply=dict(plain_us=median(w), plain_windows_us=w))
    from hidenn_fem_amd.dynamics import HyperNewmarkSolver
    from hidenn_fem_amd.modal import ModalSolver
    lin = EnergyLoss2D(E=E_SOFT, device=dev, dtype=F64, grad_convention="physical")
    lam1 = float(ModalSolver(model(), lin, n_modes=1, density=RHO, precond="amg", rtol=1e-8).solve().eigenvalues[0])
    T1 = 2.0 * math.pi / lam1 ** 0.5
    s = HyperNewmarkSolver(m, lf, T1 / 20.0, density=RHO, precond="block_jacobi")
    s.refresh()
    n, ln, L, st, P = s.n_u, s.len, _lib.lib(), _lib.stream_ptr(dev), _lib.ptr
    v = [torch.randn((n, 2), dtype=F64, device=dev, generator=g) for _ in range(11)]
    u = m.u_free.detach().to(F64).contiguous()
    pq, h = torch.empty((), dtype=F64, device=dev), s.newton._h
    call = lambda: _lib.check(L.hfem_cg_apply(h, P(v[0]), P(v[1]), P(pq), st))
    # the handle holds one binding at a time: plain and shifted alternate by rebinding between windows (outside the events)
    s.newton._u.copy_(u)
    s.newton._linearise()
    plain_a, = windows_us([call], reps)
    s.operator_apply(v[0], None, u=u)
    shifted, = windows_us([call], reps)
    s.newton._linearise()
    plain_b, = windows_us([call], reps)
    mass, = windows_us([lambda: s._mass.apply(v[0], v[2])], reps)
    plain = sorted(plain_a + plain_b)
    apply = dict(plain_us=median(plain), plain_windows_us=plain, shifted_us=median(shifted), shifted_windows_us=shifted,
                 shifted_over_plain=median(shifted) / median(plain), separate_mass_apply_us=median(mass),
                 composed_us=median(plain) + median(mass), composed_over_plain=(median(plain) + median(mass)) / median(plain),
                 folded_faster_than_composed=median(shifted) < median(plain) + median(mass),
                 order="plain (5 windows), shifted (5), plain (5): the handle is rebound between the groups")
    vec = 16 * n
    ev = lambda fn: median(windows_us([fn], reps)[0])
    vector = dict(
        trial=entry(ev(lambda: _lib.check(L.hfem_newmark_trial(0, P(v[0]), P(v[1]), P(v[2]), P(v[3]), P(v[4]), ln, 0.5, 1e-4, P(v[5]),
                                                               P(v[6]), P(v[7]), st))), 8 * vec),
        residual=entry(ev(lambda: _lib.check(L.hfem_newmark_residual(0, P(v[0]), P(v[1]), P(v[2]), P(v[3]), ln, 1.01, 0.1, 1.0,
                                                                     P(v[8]), P(v[9]), st))), 6 * vec),
        residual_without_damping_and_negative=entry(ev(lambda: _lib.check(L.hfem_newmark_residual(
            0, P(v[0]), None, P(v[2]), P(v[3]), ln, 1.0, 0.0, 1.0, P(v[8]), None, st))), 4 * vec))
    del s
    tf = lambda x: torch.stack([torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], -TRACTION)], dim=1)
    load = lambda t: 0.5 * (1.0 - math.cos(2.0 * math.pi * t / T1))
    steps = {}
    for frac in (20, 400):
        for precond in ("amg", "block_jacobi"):
            sv = HyperNewmarkSolver(model(), lf, T1 / frac, density=RHO, precond=precond, t_force=tf, load=load, rtol=1e-10,
                                    cg_max_iter=20000)
            sv.set_state()
            rec = []
            for _ in range(n_steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = sv.step(1)[0]
                torch.cuda.synchronize()
                rec.append(dict(wall_ms=1e3 * (time.perf_counter() - t0), newton=info.newton_iterations, cg=info.iterations,
                                min_J=info.min_J, reason=info.reason))
            steps[f"T1/{frac} {precond}"] = rec
            del sv
    return dict(head, free_dofs=2 * n, T1=T1, traction=TRACTION, apply=apply, vector=vector, steps=steps,
                steps_note="per step() call with its host synchronisations; rtol 1e-10, Newton from the previous a; the load rises "
                           "as (1 - cos(2 pi t / T1)) / 2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--quad", action="store_true", help="Q1M instead of T1M")
    ap.add_argument("--small", action="store_true", help="101x51 / 142x71 nodes (a check that the script runs)")
    ap.add_argument("--plain-only", action="store_true", help="the plain tangent apply alone (works on a build without the fold)")
    ap.add_argument("--lib", default="", help="another build of libhidenn_hip.so (with --plain-only)")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    if a.plain_only:                                         # a build from before this feature does not export them
        for sym in NEW_SYMBOLS:
            _lib.PROTOTYPES.pop(sym, None)
    name, quad, nx, ny = ("Q1M", True, 1415, 708) if a.quad else ("T1M", False, 1001, 501)
    if a.small:
        nx, ny = nx // 10 + 1, ny // 10 + 1
    line = json.dumps(measure(name, quad, nx, ny, a.reps, a.steps, a.plain_only))
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        tag = "_plain_" + os.path.splitext(os.path.basename(a.lib))[0] if a.plain_only and a.lib else ("_plain" if a.plain_only else "")
        with open(os.path.join(a.out_dir, f"hyper_dynamics_timing_{name}{tag}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
