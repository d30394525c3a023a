#!/usr/bin/env python3
"""The Newton-Krylov solve on the Neo-Hookean tangent, measured (dev tool; records, asserts nothing).

Launches at T1M (1001 x 501 nodes, 10^6 TRI3, fp64, jitter 0.2, left edge clamped, the finite-strain test field on the free
rows), device events around back-to-back calls on preallocated buffers, the three ALTERNATING in one process, median of 7
windows each:
  * `tangent_apply`: hfem_cg_apply on a hfem_cg_create_hyper solver (csrc/tri3_hyper_cg.hip), one-element-per-slot plan;
  * `neo_hookean_gradient`: hfem_tri3_hyper_energy_plan with HFEM_FLAG_NO_GX on the SAME plan and buffers (the residual of the
    Newton loop: tile kernel + one-block finish);
  * `linear_apply`: hfem_cg_apply of FrozenMeshSolver on the PAIRED plan of the same mesh (csrc/tri3_cg.hip).
Cache regime: the working set stays in the 256 MB Infinity Cache (same buffers every launch).

One load increment of ``python -m examples.example4 --neo-hookean`` (its mesh, material and traction; load 1 / load_steps from
the linear frozen-mesh solution): per preconditioner the Newton iterations, CG iterations and seconds of
``NewtonKrylovSolver.solve()`` (host clock, synchronised; the first solve of a solver includes its graph capture), beside the
increment as the example minimises it without ``--newton``: 100 outer ``FusedLBFGS`` steps, their seconds and the |g|inf reached.

``--quad``: the same two records for QUAD4.  Launches at DESIGN 19's Q1M (1001 x 1001 nodes, 10^6 QUAD4 cells on
[0, 2]^2, fp64, jitter 0.2, every row free, the field on every row), all three on the model's own QUAD4 plan and the same
buffers: hfem_cg_apply on the QUAD4 tangent (csrc/quad4_hyper_cg.hip), hfem_quad4_hyper_energy_plan with HFEM_FLAG_NO_GX, and
``Quad4FrozenMeshSolver``'s linear hfem_cg_apply (csrc/quad4_cg.hip).  The increment: ``example4 --neo-hookean --quad``'s plate
(no holes) with ``Quad4NewtonKrylovSolver``.  Written to newton_timing_Q1M.json.  ``--lib-tag recompute --launches-only`` runs
the launches on ``csrc/build.py --tag recompute --define HFEM_QUAD4_TANGENT_RECOMPUTE``'s library (the apply that calls log1p
instead of reading the c_q its diag launch stored) and writes newton_timing_Q1M_recompute.json: the A/B pair of DESIGN 20.

``--precond amg_tangent``: the AMG hierarchy of the assembled tangent instead of the two records above, written
to newton_amg_tangent_{T1M,Q1M}.json.  `setup`: the numeric setup of the tangent hierarchy (hfem_amg_setup_hyper) against the
small-strain one (hfem_amg_setup) on the SAME handle, alternating, device events around each call (launches only: the dense
coarsest factorisation is the host's and is timed apart, as ``_AmgDevice`` reports it), median of 7, at T1M / at Q1M with the
left edge clamped (the hierarchy needs Dirichlet rows), 0.3 x the test field.  `ramp`: the 8-step load ramp of example 4's
plates from u = 0, every increment from the last equilibrium, for ``"amg"`` against ``"amg_tangent"`` with
``amg_rebuild="newton"`` and ``"solve"`` (``--amg-rebuild`` picks one), up to the largest load that keeps min J > 0.3: Newton
iterations, CG iterations, milliseconds (device events around ``solve()``) and the fallback counts per increment.

    python scripts/newton_timing.py [--quad] [--reps 2000] [--out-dir profiles/newton] [--small] [--lib-tag TAG] [--launches-only]
                                    [--precond amg_tangent [--amg-rebuild newton|solve]]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hidenn_fem_amd import _lib
from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
from hidenn_fem_amd.mesh import generate_mesh, structured_quad_mesh, structured_tri_mesh
from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
from hidenn_fem_amd.newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver
from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver, solve_displacement_

F64 = torch.float64


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


def launches(nx, ny, reps, quad=False):
    dev = torch.device("cuda:0")
    if quad:
        coords, conn, *_ = structured_quad_mesh(nx, ny, length=2.0, height=2.0, jitter=0.2, seed=0, dtype=F64)
        m = PiecewiseLinearShapeNN2D(coords, conn)                   # DESIGN 19's Q1M: every row free
        with torch.no_grad():
            m.u_free.copy_(m.from_caller_order(field(coords), "u"))
        m = m.to(dev)
        nk = Quad4NewtonKrylovSolver(m, Quad4NeoHookeanLoss2D(device=dev, dtype=F64))
        lin = Quad4FrozenMeshSolver(m, EnergyLoss2D(device=dev, dtype=F64))
    else:
        coords, conn, geom, bc, _, edges = structured_tri_mesh(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
        m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=field(coords)[bc],
                                     neumann_edges=edges)            # the field on the Dirichlet rows too: no jump, no inversion
        with torch.no_grad():
            m.u_free.copy_(m.from_caller_order(field(coords)[~bc], "u"))
        m = m.to(dev)
        nk = NewtonKrylovSolver(m, NeoHookeanLoss2D(device=dev, dtype=F64))
        lin = FrozenMeshSolver(m, EnergyLoss2D(device=dev, dtype=F64))
    lin.refresh()
    p = torch.randn(m.u_free.shape, dtype=F64, device=dev) * 1e-4
    nk.apply(p)                                                     # refresh + linearise at the field
    q, pq = torch.empty_like(p), torch.empty((), dtype=F64, device=dev)
    L, st = _lib.lib(), _lib.stream_ptr(dev)

    def tangent():
        _lib.check(L.hfem_cg_apply(nk._h, p.data_ptr(), q.data_ptr(), pq.data_ptr(), st), "hfem_cg_apply")

    def gradient():
        nk._energy(nk._u, nk._g)

    def linear():
        _lib.check(L.hfem_cg_apply(lin._h, p.data_ptr(), q.data_ptr(), pq.data_ptr(), st), "hfem_cg_apply")

    fns = dict(tangent_apply=tangent, neo_hookean_gradient=gradient, linear_apply=linear)
    for _ in range(20):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(7):                                              # alternating windows
        for k, f in fns.items():
            t[k].append(window_us(f, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    s = nk.plan.stats
    rec = dict(mesh=f"{nx}x{ny} structured QUAD4 on [0, 2]^2, jitter 0.2, every row free" if quad
               else f"{nx}x{ny} structured TRI3, jitter 0.2, left edge clamped", n_elems=m.Nelems, n_nodes=m.Nnodes,
               n_u_rows=int(m.u_free.shape[0]), min_J=nk.info[0].item(), inverted=nk.info[1].item(),
               plan_tangent=dict(paired=bool(s["paired"]), n_tiles=s["n_tiles"], max_tile_nodes=s["max_tile_nodes"],
                                 max_tile_elems=s["max_tile_elems"], threads_per_tile=256 if quad else 512),
               plan_linear=dict(paired=bool(lin.plan.stats["paired"]), n_tiles=lin.plan.stats["n_tiles"]),
               regime="cache (working set < 256 MB Infinity Cache; back-to-back launches of the same buffers)",
               reps_per_window=reps, windows=7)
    for k in fns:
        rec[k] = dict(us=med[k], windows_us=t[k])
    rec["ratio_tangent_over_gradient"] = med["tangent_apply"] / med["neo_hookean_gradient"]
    rec["ratio_tangent_over_linear_apply"] = med["tangent_apply"] / med["linear_apply"]
    return rec


def increment(nx, ny, load_steps=8, lbfgs_steps=100, E=10e9, nu=0.3, quad=False):
    from hidenn_fem_amd.optim import FusedLBFGS
    dev = torch.device("cuda:0")
    holes = [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)]
    sides = {"up": 0, "down": 0, "right": 2, "left": 1}
    if quad:
        nodes, conn, geom, bc, _, edges = structured_quad_mesh(nx, ny, length=2.0, height=1.0, boundaries=sides)
    else:
        nodes, conn, geom, bc, _, edges = generate_mesh(2.0, 1.0, holes, sides, nx, ny)
    m = PiecewiseLinearShapeNN2D(nodes.to(F64), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(dev)
    m.node_coords_free.requires_grad_(False)
    lf = (Quad4NeoHookeanLoss2D if quad else NeoHookeanLoss2D)(E=E, nu=nu, length=2.0, height=1.0, device=dev, dtype=F64)
    solver = Quad4NewtonKrylovSolver if quad else NewtonKrylovSolver
    scale = 1.0 / load_steps
    tr = lambda x: torch.stack([torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], -scale * E / 500.0)], dim=1)
    solve_displacement_(m, EnergyLoss2D(E=E, nu=nu, device=dev, dtype=F64, grad_convention="physical"), t_force=tr, rtol=1e-10)
    u_lin = m.u_free.detach().clone()
    rec = dict(mesh=f"example 4 QUAD4 plate (no holes), {nx}x{ny} nodes" if quad else f"example 4 plate with holes, {nx}x{ny}", n_elems=m.Nelems, n_nodes=m.Nnodes, load=scale, newton={})
    for pc in ("block_jacobi", "amg", "none"):
        with torch.no_grad():
            m.u_free.copy_(u_lin)
        s = solver(m, lf, t_force=tr, precond=pc)
        s.refresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = s.solve()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        with torch.enable_grad():                                   # |g|inf as the example's L-BFGS column states it
            m.u_free.grad = None
            lf(m, None, tr).backward()
        rec["newton"][pc] = dict(newton_iterations=info.newton_iterations, cg_iterations=info.cg_iterations, seconds=sec,
                                 reason=info.reason, grad_norm_over_rhs=info.grad_norm / max(info.rhs_norm, 1e-300),
                                 g_inf=m.u_free.grad.abs().max().item(), energy=info.energy, min_J=info.min_J,
                                 cg_per_newton=[h["cg_iterations"] for h in info.history],
                                 cg_reasons=[h["cg_reason"] for h in info.history], steps=[h["step"] for h in info.history])
    with torch.no_grad():
        m.u_free.copy_(u_lin)
    opt = FusedLBFGS([m.u_free])

    def closure():
        opt.zero_grad()
        value = lf(m, None, tr)
        value.backward()
        return value

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(lbfgs_steps):
        opt.step(closure)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    value = closure()
    rec["fused_lbfgs"] = dict(steps=lbfgs_steps, seconds=sec, g_inf=m.u_free.grad.abs().max().item(), energy=value.item(),
                              min_J=float(lf.info[0]))
    return rec


def amg_setup_times(nx, ny, quad=False, windows=7):
    """Device-event medians of hfem_amg_setup_hyper against hfem_amg_setup on one handle, alternating."""
    import ctypes as C
    from hidenn_fem_amd._lib import check, ptr, stream_ptr
    dev = torch.device("cuda:0")
    mesher = structured_quad_mesh if quad else structured_tri_mesh
    coords, conn, geom, bc, _, edges = mesher(nx, ny, length=2.0, height=2.0 if quad else 1.0, jitter=0.2, seed=0, dtype=F64)
    u = 0.3 * field(coords)
    m = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=u[bc], neumann_edges=edges)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(u[~bc], "u"))
    m = m.to(dev)
    lf = (Quad4NeoHookeanLoss2D if quad else NeoHookeanLoss2D)(device=dev, dtype=F64)
    s = (Quad4NewtonKrylovSolver if quad else NewtonKrylovSolver)(m, lf, precond="amg_tangent")
    s._fresh()
    s._u.copy_(m.u_free.detach())
    s._linearise()
    a, L, st = s._amg, _lib.lib(), stream_ptr(dev)
    lam, mu = lf.lame
    mat, W = (C.c_double * 4)(lam + 2 * mu, lam, lam + 2 * mu, mu), float(lf._W)
    fixed = lambda t: ptr(t) if t.numel() else None

    def tangent():
        check(L.hfem_amg_setup_hyper(a._h, ptr(s._xf), fixed(s._xfix), ptr(s._u), fixed(s._ufix), s._lame, W, ptr(a.coarse), st),
              "hfem_amg_setup_hyper")

    def small():
        check(L.hfem_amg_setup(a._h, ptr(s._xf), fixed(s._xfix), mat, W, ptr(a.coarse), st), "hfem_amg_setup")

    fns = dict(tangent=tangent, small_strain=small)
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(window_us(f, 3))
    ok = s._amg.setup_hyper(s._xf, s._xfix, s._u, s._ufix, s._lame, W)      # with the host's Cholesky: wall seconds
    s._small_strain_setup()
    rep = s.amg
    rec = dict(mesh=f"{nx}x{ny} structured {'QUAD4 on [0, 2]^2' if quad else 'TRI3'}, jitter 0.2, left edge clamped, 0.3 x field",
               n_elems=m.Nelems, n_u_rows=int(m.u_free.shape[0]), min_J=s.info[0].item(), levels=rep["levels"], rows=rep["rows"],
               operator_complexity=rep["operator_complexity"], coarse_positive_definite=bool(ok), windows=windows,
               calls_per_window=3, wall_seconds_with_coarse_factorisation=dict(tangent=a.seconds_hyper, small_strain=a.seconds))
    for k in fns:
        rec[k] = dict(us=sorted(t[k])[len(t[k]) // 2], windows_us=t[k])
    rec["ratio_tangent_over_small_strain"] = rec["tangent"]["us"] / rec["small_strain"]["us"]
    return rec


def amg_ramp(nx, ny, quad=False, load_steps=8, E=10e9, nu=0.3, configs=None, min_j_floor=0.3):
    """Example 4's Neo-Hookean ramp from u = 0, every increment from the last equilibrium, per preconditioner configuration."""
    dev = torch.device("cuda:0")
    holes = [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)]
    sides = {"up": 0, "down": 0, "right": 2, "left": 1}
    if quad:
        nodes, conn, geom, bc, _, edges = structured_quad_mesh(nx, ny, length=2.0, height=1.0, boundaries=sides)
    else:
        nodes, conn, geom, bc, _, edges = generate_mesh(2.0, 1.0, holes, sides, nx, ny)
    lf = (Quad4NeoHookeanLoss2D if quad else NeoHookeanLoss2D)(E=E, nu=nu, length=2.0, height=1.0, device=dev, dtype=F64)
    solver = Quad4NewtonKrylovSolver if quad else NewtonKrylovSolver
    tr = lambda scale: (lambda x: torch.stack([torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], -scale * E / 500.0)], dim=1))
    rec = dict(mesh=f"example 4 QUAD4 plate (no holes), {nx}x{ny} nodes" if quad else f"example 4 plate with holes, {nx}x{ny}",
               load_steps=load_steps, min_J_floor=min_j_floor, runs={})
    for pc, rebuild in configs or (("amg", None), ("amg_tangent", "newton"), ("amg_tangent", "solve")):
        m = PiecewiseLinearShapeNN2D(nodes.to(F64), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                     neumann_edges=edges).to(dev)
        m.node_coords_free.requires_grad_(False)
        s = solver(m, lf, precond=pc, **({} if rebuild is None else dict(amg_rebuild=rebuild)))
        rows = []
        for k in range(1, load_steps + 1):
            s.t_force = tr(k / load_steps)
            s.refresh()
            before = dict(s.amg)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            info = s.solve()
            b.record()
            torch.cuda.synchronize()
            if not info.converged or info.min_J <= min_j_floor:
                rows.append(dict(load=k / load_steps, stopped=info.reason, min_J=info.min_J))
                break
            row = dict(load=k / load_steps, newton_iterations=info.newton_iterations, cg_iterations=info.cg_iterations,
                       ms=a.elapsed_time(b), min_J=info.min_J, cg_per_newton=[h["cg_iterations"] for h in info.history])
            if pc == "amg_tangent":
                after = s.amg
                row.update({key: after[key] - before[key] for key in ("tangent_setups", "fallbacks_coarse", "fallbacks_descent")})
            rows.append(row)
        rec["runs"][pc if rebuild is None else f"{pc}/{rebuild}"] = rows
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--small", action="store_true", help="101x51 / 60x30 nodes (a check that the script runs)")
    ap.add_argument("--quad", action="store_true", help="Q1M and example 4's QUAD4 plate: the QUAD4 tangent (DESIGN 20)")
    ap.add_argument("--lib-tag", default="", help="run on csrc/libhidenn_hip_<tag>.so (csrc/build.py --tag: an A/B build)")
    ap.add_argument("--launches-only", action="store_true", help="skip the load increment")
    ap.add_argument("--precond", choices=["amg_tangent"], default=None,
                    help="amg_tangent: measure the AMG hierarchy of the assembled tangent instead (DESIGN 21)")
    ap.add_argument("--amg-rebuild", choices=["newton", "solve"], default=None,
                    help="with --precond amg_tangent: only this rebuild setting in the ramp (default: both, beside 'amg')")
    a = ap.parse_args()
    big = not a.small
    if a.lib_tag:
        _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"libhidenn_hip_{a.lib_tag}.so")
    if a.precond == "amg_tangent":
        cfg = None if a.amg_rebuild is None else (("amg", None), ("amg_tangent", a.amg_rebuild))
        rec = dict(setup=amg_setup_times(*(((1001, 1001) if a.quad else (1001, 501)) if big else ((101, 101) if a.quad else (101, 51))),
                                         quad=a.quad),
                   ramp=amg_ramp(*((200, 100) if big else (60, 30)), quad=a.quad, configs=cfg))
    elif a.launches_only:
        rec = dict(launches=launches(*(((1001, 1001) if a.quad else (1001, 501)) if big else ((101, 101) if a.quad else (101, 51))),
                                     a.reps, quad=a.quad))
    elif a.quad:
        rec = dict(launches=launches(*((1001, 1001) if big else (101, 101)), a.reps, quad=True),
                   increment=increment(*((200, 100) if big else (60, 30)), quad=True))
    else:
        rec = dict(launches=launches(*((1001, 501) if big else (101, 51)), a.reps),
                   increment=increment(*((200, 100) if big else (60, 30))))
    rec["library"] = a.lib_tag or "product"
    line = json.dumps(rec)
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        name = ("newton_timing_Q1M" if a.quad else "newton_timing_T1M") if big else "newton_timing_small"
        if a.precond == "amg_tangent":
            name = ("newton_amg_tangent_Q1M" if a.quad else "newton_amg_tangent_T1M") if big else "newton_amg_tangent_small"
        with open(os.path.join(a.out_dir, name + (f"_{a.lib_tag}" if a.lib_tag else "") + ".json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
