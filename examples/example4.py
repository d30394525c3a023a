"""Example 4 -- 2D plate with holes under traction, linear elasticity, r-adaptivity, LBFGS
(reference examples/example4.py: plate 2x1, three holes, left edge Dirichlet, right edge Neumann,
E=10e9, nu=0.3, 30 LBFGS outer steps).  Mesh from this repo's structured mesher (the reference's
commented alternative, example4.py:27); every closure call is ONE fused kernel launch."""
import argparse

import torch

from src.loss import EnergyLoss2D
from src.mesh import generate_mesh
from src.models import PiecewiseLinearShapeNN2D


def run(nx=200, ny=100, steps=30, dtype=torch.float32, log_every=5, fused_lbfgs=False, sharded=False, solve_first=False,
        r_adapt=False, outer=20, precond="block_jacobi", quad=False, error_estimate=False, modes=0, dynamics=0, dt=None,
        buckling=0, harmonic=0, topopt=0):
    """``sharded=True``: the same loop OWNER-SHARDED over the ranks of the process group (one process per GPU:
    ``python -m torch.distributed.run --nproc-per-node N examples/example4.py --sharded``; a single process works too): elements
    are split into per-rank tile ranges and L-BFGS itself is node-sharded (``hidenn_fem_amd.optim.ShardedLBFGS``: every rank keeps
    the history and direction of the rows its tiles own; two small exchanges per inner iteration).
    ``solve_first=True``: before the loop, ``u_free`` is set to the displacement that minimises the energy on the initial mesh
    (``hidenn_fem_amd.solve.solve_displacement_``: preconditioned CG at frozen coordinates) and that energy is printed -- the
    fixed-mesh FEM reference an r-adapted energy is compared against.  The L-BFGS loop then starts from it; with the reference's
    fixed step (lr 1, no line search) on coordinates and displacements together it does not stay there: at that point the
    gradient is all coordinate gradient, and the coordinate steps invert elements (the energy turns NaN on this plate; the
    reference's own op chain does the same on a smaller plate on the CPU).
    ``r_adapt=True``: the alternating scheme the reference sketches in comments (example4.py:83-110) instead of the L-BFGS loop:
    the frozen-mesh solve, then ``outer`` iterations of ``hidenn_fem_amd.radapt.RAdaptiveSolver`` (re-solve ``u``, an L-BFGS step
    on the coordinates bounded so that no element inverts, Armijo on the energy); prints the energy history, the smallest
    element quality and the stopping reason, and returns the r-adapted energy ``Pi*``.
    ``precond``: the CG preconditioner of ``solve_first`` and ``r_adapt`` (``"block_jacobi"`` or ``"amg"``).
    ``quad=True`` (with ``r_adapt``): the same plate without the holes as ``nx x ny`` nodes of bilinear QUAD4 cells
    (``structured_quad_mesh``: the structured mesher cuts holes into triangles only), same sides, material and traction, run
    through ``hidenn_fem_amd.radapt.r_adapt_`` (``Quad4RAdaptiveSolver``); prints the same three kinds of line.
    ``error_estimate=True``: prints the relative ZZ error estimate eta_rel (``hidenn_fem_amd.post.StressRecovery``: recovered
    nodal stress, energy-norm indicator) after the solve and, with ``r_adapt``, on the frozen mesh and on the r-adapted one.
    The estimate measures the discretisation error only in the physical gradient convention, so under this switch the loss is
    built with ``grad_convention="physical"`` (and the run says so): the energies then differ from the reference convention's.
    ``modes=N`` (``--modes N``, N <= 8): after the mesh is built, prints the N lowest free-vibration frequencies of the plate
    (``hidenn_fem_amd.modal.vibration_modes``: block LOBPCG on ``K phi = lambda M phi`` with the consistent mass, unit density,
    preconditioner ``precond``) and returns ``(model, ModalInfo)``; nothing else runs.  The loss is built with
    ``grad_convention="physical"``, where the frequencies are those of the elastic plate; ``quad=True`` gives the QUAD4 plate.
    ``dynamics=N`` (``--dynamics N``): a step load on the plate at rest -- the default traction switched on at t = 0 -- followed
    for N Newmark steps (``hidenn_fem_amd.dynamics.NewmarkSolver``: average acceleration, consistent mass, unit density,
    preconditioner ``precond``), printing t, the tip displacement, the CG iterations and the total energy of every step;
    ``dt`` (``--dt``) defaults to 1/20 of the lowest mode's period (one ``vibration_modes`` solve).  Physical convention;
    returns ``(model, [StepInfo])``; nothing else runs.
    ``buckling=N`` (``--buckling N``, N <= 8): the default traction REVERSED into compression; the frozen-mesh solve under it,
    then the N smallest buckling load factors about that state (``hidenn_fem_amd.buckling.linear_buckling``: block LOBPCG on
    ``K_G phi = theta K phi``, preconditioner ``precond``), printing ``lambda_j`` and the critical load
    ``P_cr = lambda_1 |sum b_x|`` from the nodal load actually applied.  Physical convention, and for the triangles
    ``gauss_order=1`` (weights that sum to the triangle's area), where the factors are those of the elastic plate; one GPU;
    returns ``(model, BucklingInfo)``; nothing else runs.
    ``harmonic=N`` (``--harmonic N``, N >= 2): the steady-state response of the plate to the default traction oscillating at N
    frequencies from half the first natural frequency to 1.1 times the third (one ``vibration_modes`` solve for the three),
    with Rayleigh damping of 2 % at the first and the third (``hidenn_fem_amd.harmonic.HarmonicSolver``: COCG on
    ``K + i omega C - omega^2 M``, consistent mass, unit density, preconditioner ``precond``, each frequency warm-started from
    the previous one), printing omega, the tip amplitude and phase and the iterations of every frequency.  Physical convention;
    one GPU; returns ``(model, [HarmonicInfo])``; nothing else runs.
    ``topopt=N`` (``--topopt N``): N design iterations of density-based (SIMP) compliance minimisation of the plate under the
    default traction (``hidenn_fem_amd.topopt.TopologyOptimizer``: volume fraction 0.4, penal 3, density filter of 1.5 mean
    element sizes, optimality-criteria update with its bisection on the device, preconditioner ``precond``), printing the
    compliance, the volume, the change, the PCG iterations and the multiplier of every iteration.  Physical convention; one
    GPU; ``quad=True`` gives the QUAD4 plate; returns ``(model, TopologyOptimizer, [TopOptInfo])``; nothing else runs."""
    import os
    import torch.distributed as dist
    if buckling and (sharded or modes or dynamics):
        raise NotImplementedError("example 4: buckling=N / --buckling N runs on one GPU and on its own; drop --sharded / --modes "
                                  "/ --dynamics")
    if topopt and (sharded or modes or dynamics or buckling or harmonic):
        raise NotImplementedError("example 4: topopt=N / --topopt N runs on one GPU and on its own; drop --sharded / --modes "
                                  "/ --dynamics / --buckling / --harmonic")
    if harmonic and (sharded or modes or dynamics or buckling):
        raise NotImplementedError("example 4: harmonic=N / --harmonic N runs on one GPU and on its own; drop --sharded / --modes "
                                  "/ --dynamics / --buckling")
    if modes and sharded:
        raise NotImplementedError("example 4: modes=N / --modes N runs on one GPU (the modal solver is not sharded); drop "
                                  "sharded=True / --sharded")
    if dynamics and (sharded or modes):
        raise NotImplementedError("example 4: dynamics=N / --dynamics N runs on one GPU and on its own; drop --sharded / --modes")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local % max(torch.cuda.device_count(), 1)) if sharded else torch.device("cuda")
    if sharded and "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1 and not dist.is_initialized():
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", device_id=dev)
    rank0 = (not sharded) or not dist.is_initialized() or dist.get_rank() == 0
    length, height = 2.0, 1.0
    holes = [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)]
    sides = {"up": 0, "down": 0, "right": 2, "left": 1}
    if quad:
        if not r_adapt and not modes and not dynamics and not buckling and not harmonic and not topopt:
            raise NotImplementedError("example 4: quad=True runs the r-adaptive solve, the modes, the dynamics, the buckling, "
                                      "the harmonic analysis or the topology optimisation only (pass r_adapt=True / --r-adapt, "
                                      "modes=N / --modes N, dynamics=N / --dynamics N, buckling=N / --buckling N, harmonic=N / "
                                      "--harmonic N or topopt=N / --topopt N)")
        from hidenn_fem_amd.mesh import structured_quad_mesh
        nodes, conn, geom, bc, mn, edges = structured_quad_mesh(nx, ny, length=length, height=height, boundaries=sides)
    else:
        nodes, conn, geom, bc, mn, edges = generate_mesh(length, height, holes, sides, nx, ny)
    if rank0:
        print(f"nodes {tuple(nodes.shape)} elements {tuple(conn.shape)} boundary {int(geom.sum())} "
              f"dirichlet {int(bc.sum())} neumann edges {tuple(edges.shape)}")
    if sharded:
        torch.manual_seed(0)                                       # every rank must draw the same initial u_free
    model = PiecewiseLinearShapeNN2D(nodes.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                     neumann_edges=edges).to(dev)
    loss_fn = EnergyLoss2D(E=10e9, nu=0.3, length=length, height=height, device=dev, dtype=dtype,
                           grad_convention="physical" if (error_estimate or modes or dynamics or buckling or harmonic or topopt) else None,
                           **(dict(gauss_order=1) if buckling else {}))
    if buckling:
        return _buckling(model, loss_fn, buckling, precond)
    if harmonic:
        return _harmonic(model, loss_fn, harmonic, precond)
    if topopt:
        return _topopt(model, loss_fn, topopt, precond)
    if modes:
        return _modes(model, loss_fn, modes, precond, rank0)
    if dynamics:
        return _dynamics(model, loss_fn, dynamics, dt, precond)
    if error_estimate and rank0:
        print('error estimate: the loss uses grad_convention="physical" (eta estimates the discretisation error only there)')
    if r_adapt:
        return _r_adapt(model, loss_fn, outer, precond, error_estimate)
    if solve_first:
        import time
        from hidenn_fem_amd.solve import solve_displacement_
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = solve_displacement_(model, loss_fn, rtol=1e-10, precond=precond)
        torch.cuda.synchronize()
        if rank0:
            print(f"frozen-mesh solve: {info.iterations} CG iterations, |r|/|f| = {info.residual_norm / max(info.rhs_norm, 1e-300):.2e} "
                  f"({info.reason}), {time.perf_counter() - t0:.3f} s, energy {loss_fn(model).item():.6e}")
            if error_estimate:
                _print_error(model, loss_fn, "after the frozen-mesh solve")
    if sharded:
        import time
        from hidenn_fem_amd.optim import ShardedLBFGS
        from hidenn_fem_amd.sharded import LibraryComm, ShardedTri3Energy
        comm = LibraryComm(dev) if dist.is_initialized() and dist.get_world_size() > 1 else None     # in-library RCCL: capturable
        sh = ShardedTri3Energy(model, loss_fn, comm=comm).setup_interfaces()
        opt = ShardedLBFGS(sh)                                                                       # torch.optim.LBFGS defaults
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for step in range(steps):
            value = opt.step()
            if rank0 and step % log_every == 0:
                print(f"Epoch {step:04d}: Loss = {value.item():.6e}")
        opt.finish()
        torch.cuda.synchronize()
        if rank0:
            print(f"{opt.state['func_evals']} closure calls, final loss {value.item():.6e}, {time.perf_counter() - t0:.3f} s "
                  f"(ShardedLBFGS over {sh.world} rank(s), {opt._n} of {model.node_coords_free.numel() + model.u_free.numel()} parameters here)")
            if error_estimate:
                _print_error(model, loss_fn, "after the loop")
        return model, value.item()
    if fused_lbfgs:                      # same algorithm and defaults, device-resident (hidenn_fem_amd/optim.py)
        from hidenn_fem_amd.optim import FusedLBFGS
        opt = FusedLBFGS(model.parameters())
    else:
        opt = torch.optim.LBFGS(model.parameters())
    calls = [0]

    def closure():
        calls[0] += 1
        if fused_lbfgs:                   # autograd-free: one launch writes loss and .grad (no zero_grad / backward)
            return loss_fn.value_and_grad_(model)
        opt.zero_grad()
        value = loss_fn(model)
        value.backward()
        return value

    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(steps):
        value = opt.step(closure)
        if step % log_every == 0:
            print(f"Epoch {step:04d}: Loss = {value.item():.6e}")
    torch.cuda.synchronize()
    print(f"{calls[0]} closure calls, final loss {value.item():.6e}, {time.perf_counter() - t0:.3f} s "
          f"({'FusedLBFGS' if fused_lbfgs else 'torch.optim.LBFGS'})")
    if error_estimate:
        _print_error(model, loss_fn, "after the loop")
    return model, value.item()


def run_neo_hookean(nx=200, ny=100, steps=100, dtype=torch.float64, load_steps=8, E=10e9, nu=0.3, newton=False,
                    precond="block_jacobi", quad=False, r_adapt=False, outer=10, error_estimate=False, dynamics=0, dt=None):
    """The plate at FINITE strain (``--neo-hookean``): compressible Neo-Hookean material (``NeoHookeanLoss2D``), left edge
    clamped, the right edge pulled DOWN by the dead traction ``(0, -E/500)`` -- a tip deflection of about a third
    of the height.  The mesh is frozen; the load is ramped in ``load_steps`` increments and each increment is minimised over
    ``u_free`` by ``steps`` outer ``FusedLBFGS`` steps, started from the previous state scaled to the new load (the first one:
    from the linear frozen-mesh solve).  An increment after which an element is inverted (``loss_fn.info[1] > 0``) or the
    energy is not finite is taken back and halved.  Prints energy, min J and the tip deflection per load step and, at the
    smallest load, the gap to the linear solution.  Returns ``(model, energy)``.
    ``newton=True`` (``--newton``): the same ramp, predictor and halving rule, each increment solved to equilibrium by
    ``hidenn_fem_amd.newton.NewtonKrylovSolver`` (inexact Newton, truncated PCG on the tangent, preconditioner ``precond``)
    instead of ``FusedLBFGS``; the line then also shows the Newton and CG iterations (``precond="amg_tangent"``, the AMG
    hierarchy of the assembled tangent rebuilt at every linearisation: also the number of tangent setups and of fallbacks
    to the small-strain hierarchy, coarse / descent).  An increment whose Newton solve does not converge is taken back and
    halved like an inverted one.
    ``quad=True`` (``--quad``): the same ramp on the plate without the holes as ``nx x ny`` nodes of bilinear QUAD4 cells
    (``structured_quad_mesh``), with ``Quad4NeoHookeanLoss2D``; with ``newton=True`` every increment is solved by
    ``Quad4NewtonKrylovSolver``.
    ``r_adapt=True`` (``--r-adapt``): the Newton ramp to the full load as above (``newton`` is implied), then ``outer``
    iterations of the finite-strain r-adaptive solve there (``hidenn_fem_amd.radapt.r_adapt_``: ``HyperRAdaptiveSolver`` /
    ``Quad4HyperRAdaptiveSolver`` -- Newton-Krylov with ``precond`` for ``u``, coordinate steps bounded so that neither an
    element nor its ``det F`` collapses); prints energy, min J, min q and the Newton / CG counts per outer iteration and the
    energy gained over the frozen mesh, and returns the r-adapted energy.
    ``error_estimate=True`` (``--error-estimate``): after every converged load increment one line with the relative ZZ error
    indicator eta_rel, min J and the largest nodal von Mises stress of the recovered CAUCHY stress
    (``hidenn_fem_amd.post.HyperStressRecovery`` -- an indicator, not an estimate, away from small strain: DESIGN 24); with
    ``r_adapt`` also on the frozen mesh and on the r-adapted one, all from one reused object.

    ``dynamics=N`` (``--dynamics N``): no ramp; a step load on the plate at rest -- a tenth of the ramp's full traction switched
    on at t = 0 -- followed for N Newmark steps at finite strain (``hidenn_fem_amd.dynamics.HyperNewmarkSolver``: average
    acceleration, consistent mass, unit density, one Newton-Krylov solve per step with preconditioner ``precond``), printing t,
    the tip displacement, the Newton and CG iterations, min J and the total energy of every step; ``dt`` defaults to 1/20 of the
    period of the lowest mode of the linearised plate.  Returns ``(model, [HyperStepInfo])``."""
    newton = newton or r_adapt
    from hidenn_fem_amd.loss import NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    from hidenn_fem_amd.optim import FusedLBFGS
    from hidenn_fem_amd.solve import solve_displacement_
    dev = torch.device("cuda")
    length, height = 2.0, 1.0
    holes = [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)]
    sides = {"up": 0, "down": 0, "right": 2, "left": 1}
    if quad:
        from hidenn_fem_amd.mesh import structured_quad_mesh
        nodes, conn, geom, bc, mn, edges = structured_quad_mesh(nx, ny, length=length, height=height, boundaries=sides)
    else:
        nodes, conn, geom, bc, mn, edges = generate_mesh(length, height, holes, sides, nx, ny)
    print(f"nodes {tuple(nodes.shape)} elements {tuple(conn.shape)} dirichlet {int(bc.sum())} neumann edges {tuple(edges.shape)}")
    model = PiecewiseLinearShapeNN2D(nodes.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                     neumann_edges=edges).to(dev)
    model.node_coords_free.requires_grad_(False)                   # frozen mesh: the launch skips the coordinate gradient
    loss_fn = (Quad4NeoHookeanLoss2D if quad else NeoHookeanLoss2D)(E=E, nu=nu, length=length, height=height, device=dev, dtype=dtype)
    tau = E / 500.0
    tip = torch.nonzero(model.from_caller_order(nodes[~bc][:, 0:1].to(dev), "u")[:, 0] > length - 1e-6)[:, 0]

    def traction(scale):
        return lambda x: torch.stack([torch.zeros_like(x[:, 0]), torch.full_like(x[:, 0], -scale * tau)], dim=1)

    if dynamics:
        if precond == "amg_tangent":
            raise NotImplementedError("example 4: --neo-hookean --dynamics takes --precond block_jacobi or amg")
        lin = EnergyLoss2D(E=E, nu=nu, length=length, height=height, device=dev, dtype=dtype, grad_convention="physical")
        return _hyper_dynamics(model, loss_fn, lin, traction(0.1), dynamics, dt, precond)

    def minimise(scale):
        opt = FusedLBFGS([model.u_free])
        t = traction(scale)

        def closure():
            opt.zero_grad()
            value = loss_fn(model, None, t)
            value.backward()
            return value

        for _ in range(steps):
            opt.step(closure)
        with torch.no_grad():
            value = loss_fn(model, None, t)
        return value.item(), float(loss_fn.info[0]), int(loss_fn.info[1]), model.u_free.grad.abs().max().item()

    def equilibrium(scale):
        from hidenn_fem_amd.newton import NewtonKrylovSolver, Quad4NewtonKrylovSolver
        solver = Quad4NewtonKrylovSolver if quad else NewtonKrylovSolver
        s = solver(model, loss_fn, t_force=traction(scale), precond=precond)
        info = s.solve()
        ginf = float("inf") if not info.converged else info.grad_norm       # an unconverged increment is taken back
        return info.energy, info.min_J, 0 if info.converged else 1, ginf, info, s.amg if precond == "amg_tangent" else None

    recovery = None
    done, inc, first = 0.0, 1.0 / load_steps, True
    energy = float("nan")
    prev, prev_load = torch.zeros_like(model.u_free), 0.0          # the accepted state before the last one (secant predictor)
    while done < 1.0 - 1e-12 and inc > 1e-4:
        target = min(1.0, done + inc)
        keep = model.u_free.detach().clone()
        with torch.no_grad():
            if first:
                lin = EnergyLoss2D(E=E, nu=nu, length=length, height=height, device=dev, dtype=dtype, grad_convention="physical")
                solve_displacement_(model, lin, t_force=traction(target), rtol=1e-10)
                u_lin = model.u_free.detach().clone()
            else:                                                  # along the secant through the last two accepted states
                model.u_free.add_((keep - prev) * ((target - done) / (done - prev_load)))
        if newton:
            value, min_j, inverted, ginf, ninfo, amg = equilibrium(target)
        else:
            value, min_j, inverted, ginf = minimise(target)
        if inverted > 0 or value != value or value in (float("inf"), float("-inf")):
            with torch.no_grad():
                model.u_free.copy_(keep)
            inc *= 0.5
            what = f"Newton stopped with {ninfo.reason!r}" if newton else f"{inverted} inverted element(s)"
            print(f"load {target:.4f}: {what}, energy {value:.6e} -- increment halved to {inc:.4f}")
            continue
        prev, prev_load = keep if not first else torch.zeros_like(keep), done
        energy, done = value, target
        defl = model.u_free.detach()[tip, 1].mean().item()
        if newton:
            print(f"load {target:.4f}: energy {value:.9e} min J {min_j:.4f} tip deflection {defl:+.4f} |g|2 {ginf:.3e} "
                  f"Newton {ninfo.newton_iterations} CG {ninfo.cg_iterations}"
                  + ("" if amg is None else f" tangent setups {amg['tangent_setups']} fallbacks coarse "
                     f"{amg['fallbacks_coarse']} descent {amg['fallbacks_descent']}"))
        else:
            print(f"load {target:.4f}: energy {value:.9e} min J {min_j:.4f} tip deflection {defl:+.4f} |g|inf {ginf:.3e}")
        if first:
            gap = (model.u_free.detach() - u_lin).abs().max().item() / u_lin.abs().max().item()
            print(f"load {target:.4f}: gap to the linear frozen-mesh solution max|u - u_lin| / max|u_lin| = {gap:.3e}")
            first = False
        if error_estimate:
            recovery = _print_hyper_error(model, loss_fn, f"at load {target:.4f}", recovery)
    if r_adapt:
        if done < 1.0 - 1e-12:
            raise RuntimeError(f"example 4: the load ramp stopped at {done:.4f}; no r-adaptation below the full load")
        return _r_adapt_neo_hookean(model, loss_fn, traction(1.0), outer, precond, recovery)
    return model, energy


def run_plasticity(nx=200, ny=100, n_steps=4, dtype=torch.float64, precond="block_jacobi", sigma_y=4e5, hardening=5e8):
    """The plate with holes under the default traction as an elastoplastic load path (``--plasticity N``): small-strain J2
    plasticity with linear isotropic hardening in plane strain (``hidenn_fem_amd.plasticity.J2PlasticityLoss2D``: E = 10e9,
    nu = 0.3, yield stress ``sigma_y``, hardening modulus ``hardening``), the load ramped up to 1 in N steps and back down to
    0 in N steps, every step solved by ``ElastoplasticSolver`` (Newton-Krylov on the consistent tangent, preconditioner
    ``precond``).  Prints the Newton and CG iterations, the share of elements yielding in the step, the largest accumulated
    plastic strain and the tip displacement per step; after unloading the plate keeps a residual displacement.  Returns
    ``(model, [NewtonInfo])``."""
    import time
    from hidenn_fem_amd.plasticity import ElastoplasticSolver, J2PlasticityLoss2D
    if n_steps < 1:
        raise ValueError("example 4: plasticity=N / --plasticity N needs N >= 1 load steps each way")
    dev = torch.device("cuda")
    length, height = 2.0, 1.0
    holes = [(0.5, 0.7, 0.12), (1.0, 0.3, 0.15), (1.4, 0.6, 0.1)]
    sides = {"up": 0, "down": 0, "right": 2, "left": 1}
    nodes, conn, geom, bc, mn, edges = generate_mesh(length, height, holes, sides, nx, ny)
    print(f"nodes {tuple(nodes.shape)} elements {tuple(conn.shape)} dirichlet {int(bc.sum())} neumann edges {tuple(edges.shape)}")
    model = PiecewiseLinearShapeNN2D(nodes.to(dtype), conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0,
                                     neumann_edges=edges).to(dev)
    loss_fn = J2PlasticityLoss2D(E=10e9, nu=0.3, sigma_y=sigma_y, hardening=hardening, length=length, height=height, device=dev,
                                 dtype=dtype, gauss_order=1)   # weights that sum to the triangle's area
    with torch.no_grad():
        model.u_free.zero_()
    solver = ElastoplasticSolver(model, loss_fn, precond=precond, rtol=1e-8)
    x = model.coords.detach()[model._idx_ufree.to(model.coords.device)]
    tip = int(torch.argmax(x[:, 0] - 1e-3 * (x[:, 1] - 0.5 * x[:, 1].max()).abs()))
    print(f"J2 plasticity, plane strain: sigma_y {sigma_y:g}, hardening {hardening:g}, {precond}; load 0 -> 1 -> 0 in "
          f"{n_steps} + {n_steps} steps; tip = free row {tip}")
    loads = [(k + 1) / n_steps for k in range(n_steps)] + [(n_steps - 1 - k) / n_steps for k in range(n_steps)]
    infos = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for load in loads:
        info = solver.solve(load)
        infos.append(info)
        alpha = solver.state()[1].max().item()
        u = model.u_free.detach()[tip]
        print(f"load {load:.4f}: Newton {info.newton_iterations:2d} CG {info.cg_iterations:5d} ({info.reason}) plastic fraction "
              f"{solver.plastic_fraction:.4f} max alpha {alpha:.4e} tip u ({u[0].item():+.6e}, {u[1].item():+.6e})")
    torch.cuda.synchronize()
    print(f"{len(loads)} load steps, {sum(i.newton_iterations for i in infos)} Newton and {sum(i.cg_iterations for i in infos)} CG "
          f"iterations, {time.perf_counter() - t0:.3f} s")
    return model, infos


def _print_hyper_error(model, loss_fn, when, recovery=None):
    """One line with the finite-strain ZZ indicator; returns the ``HyperStressRecovery`` (reusable: the connectivity never
    changes, coordinates and displacements are read on every call)."""
    from hidenn_fem_amd.post import HyperStressRecovery
    recovery = recovery or HyperStressRecovery(model, loss_fn)
    err = recovery.error()
    s = err.nodal_stress
    vm = torch.sqrt(s[:, 0] ** 2 - s[:, 0] * s[:, 1] + s[:, 1] ** 2 + 3.0 * s[:, 2] ** 2).max().item()
    print(f"ZZ error indicator {when}: eta_rel {err.relative:.6e} min_J {err.min_J:.4f} max nodal von Mises {vm:.6e}")
    return recovery


def _r_adapt_neo_hookean(model, loss_fn, t_force, outer, precond, recovery=None):
    import time
    from hidenn_fem_amd.radapt import mesh_quality, quad4_mesh_quality, r_adapt_
    quality = quad4_mesh_quality if getattr(model, "nodes_per_element", 3) == 4 else mesh_quality
    model.node_coords_free.requires_grad_(True)                    # the ramp froze the mesh
    if recovery is not None:
        _print_hyper_error(model, loss_fn, "on the frozen mesh", recovery)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = r_adapt_(model, loss_fn, t_force=t_force, max_outer=outer, precond=precond)     # (Quad4)HyperRAdaptiveSolver
    torch.cuda.synchronize()
    print(f"frozen-mesh energy {info.energy[0]:.9e} min J {info.min_J[0]:.4f} min q {info.min_q[0]:.4f} "
          f"(Newton {info.newton_iterations[0]} CG {info.cg_iterations[0]})")
    for k in range(1, info.iterations + 1):
        print(f"outer {k:3d}: energy {info.energy[k]:.9e} min J {info.min_J[k]:.4f} min q {info.min_q[k]:.4f} "
              f"|g_x|inf {info.grad_inf[k]:.3e} alpha {info.alpha[k]:.3e} (max {info.alpha_max[k]:.3e}) "
              f"Newton {info.newton_iterations[k]} CG {info.cg_iterations[k]}")
    mq = quality(model)
    gain = info.energy[0] - info.energy[-1]
    print(f"r-adapted energy {info.energy[-1]:.9e} after {info.iterations} outer iterations ({info.reason}), "
          f"min J {info.min_J[-1]:.4f}, min q {mq.min_q:.4f}, inverted elements {mq.n_inverted}, {time.perf_counter() - t0:.3f} s")
    print(f"energy gained over the frozen mesh {gain:.6e} ({gain / abs(info.energy[0]):.3e} of |Pi*|)")
    if recovery is not None:
        _print_hyper_error(model, loss_fn, "on the r-adapted mesh", recovery)
    return model, info.energy[-1]


def _modes(model, loss_fn, n_modes, precond, rank0=True):
    import time
    from hidenn_fem_amd.modal import vibration_modes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = vibration_modes(model, loss_fn, n_modes=n_modes, precond=precond, max_iter=200 if precond == "amg" else 5000)
    torch.cuda.synchronize()
    if rank0:
        print(f"free vibration (consistent mass, density 1, {precond}): {info.iterations} LOBPCG iterations, "
              f"converged {info.converged}, {time.perf_counter() - t0:.3f} s")
        for j in range(n_modes):
            lam, f, r = info.eigenvalues[j].item(), info.frequencies[j].item(), info.residual_norms[j].item()
            print(f"mode {j + 1}: frequency {f:.6e} (lambda {lam:.6e}, |K x - lambda M x| {r:.3e})")
    return model, info


def _buckling(model, loss_fn, n_modes, precond):
    import time
    from hidenn_fem_amd.buckling import linear_buckling
    from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver
    t_force = lambda x: -loss_fn.uniform_edge_force(x)                     # the default traction reversed into compression
    cls = Quad4FrozenMeshSolver if getattr(model, "nodes_per_element", 3) == 4 else FrozenMeshSolver
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    static = cls(model, loss_fn, t_force=t_force, precond=precond, rtol=1e-10)
    sinfo = static.solve()                                                 # writes u_free: the prestress state
    load_x = float(static._gz[:, 0].sum().abs())                           # g_zero = dE/du at u = 0 = minus the nodal load b
    info = linear_buckling(model, loss_fn, n_modes=n_modes, precond=precond, max_iter=200 if precond == "amg" else 5000)
    torch.cuda.synchronize()
    print(f"linear buckling under the reversed traction ({precond}): {sinfo.iterations} CG iterations ({sinfo.reason}), "
          f"{info.iterations} LOBPCG iterations, converged {info.converged}, {info.n_buckling} of {n_modes} modes buckle, "
          f"{time.perf_counter() - t0:.3f} s")
    for j in range(n_modes):
        th, lam, r = info.theta[j].item(), info.load_factors[j].item(), info.residual_norms[j].item()
        print(f"mode {j + 1}: load factor {lam:.6e} (theta {th:.6e}, |K_G x - theta K x| {r:.3e})")
    print(f"nodal load |sum b_x| = {load_x:.6e}; critical load P_cr = lambda_1 |sum b_x| = {info.load_factors[0].item() * load_x:.6e}")
    return model, info


def _harmonic(model, loss_fn, n_freq, precond):
    import cmath
    import time
    from hidenn_fem_amd.harmonic import HarmonicSolver
    from hidenn_fem_amd.modal import vibration_modes
    if n_freq < 2:
        raise ValueError("example 4: harmonic=N / --harmonic N needs N >= 2 frequencies")
    lam = vibration_modes(model, loss_fn, n_modes=3, precond=precond, max_iter=200 if precond == "amg" else 5000).eigenvalues
    w1, w2, w3 = (lam[j].item() ** 0.5 for j in range(3))
    zeta = 0.02
    rayleigh = (2.0 * zeta * w1 * w3 / (w1 + w3), 2.0 * zeta / (w1 + w3))    # zeta at omega_1 and omega_3
    print(f"natural frequencies omega_1..3 = {w1:.6e}, {w2:.6e}, {w3:.6e}; Rayleigh damping {zeta:.0%} at omega_1 and omega_3: "
          f"alpha_R {rayleigh[0]:.6e}, beta_R {rayleigh[1]:.6e}")
    solver = HarmonicSolver(model, loss_fn, rayleigh=rayleigh, precond=precond)
    x = model.coords.detach()[model._idx_ufree.to(model.coords.device)]                 # node of every free u row (storage order)
    tip = int(torch.argmax(x[:, 0] - 1e-3 * (x[:, 1] - 0.5 * x[:, 1].max()).abs()))     # right edge, nearest mid-height
    print(f"harmonic response to the default traction (consistent mass, density 1, {precond}); tip = free row {tip} at "
          f"({x[tip, 0].item():.3f}, {x[tip, 1].item():.3f})")
    omegas = [0.5 * w1 + (1.1 * w3 - 0.5 * w1) * k / (n_freq - 1) for k in range(n_freq)]

    def show(omega, u, info):
        ux = complex(u[tip, 0].item())
        print(f"omega {omega:.6e} ({omega / w1:6.3f} omega_1): tip |u_x| {abs(ux):.6e} phase {cmath.phase(ux):+.4f} |u_y| "
              f"{abs(complex(u[tip, 1].item())):.6e} COCG {info.iterations:5d} ({info.reason})")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, infos = solver.sweep(omegas, rows=[tip], callback=show)
    torch.cuda.synchronize()
    print(f"{n_freq} frequencies, {sum(i.iterations for i in infos)} COCG iterations, {time.perf_counter() - t0:.3f} s")
    return model, infos


def _topopt(model, loss_fn, n_iter, precond):
    import time
    from hidenn_fem_amd.topopt import TopologyOptimizer
    with torch.no_grad():
        model.u_free.zero_()
    opt = TopologyOptimizer(model, loss_fn, 0.4, precond=precond)
    print(f"SIMP compliance minimisation under the default traction: volume fraction 0.4, penal 3, filter radius "
          f"{opt.filter_radius:.4e} (1.5 mean element sizes), e_min {opt.e_min:g}, move {opt.move:g}, {precond}")
    total = float(opt.volumes.sum())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    infos = []
    for k in range(n_iter):
        info = opt.step()
        infos.append(info)
        print(f"iteration {k + 1:4d}: compliance {info.compliance:.6e} volume fraction {info.volume / total:.6f} change "
              f"{info.change:.4f} PCG {info.iterations:5d} lambda {info.lam:.4e}" + ("" if info.feasible else " INFEASIBLE"))
    torch.cuda.synchronize()
    rf = opt.filtered_density
    print(f"{n_iter} design iterations, {sum(i.iterations for i in infos)} PCG iterations, {time.perf_counter() - t0:.3f} s; "
          f"grey elements (0.1 < rho~ < 0.9): {int(((rf > 0.1) & (rf < 0.9)).sum())} of {rf.numel()}")
    return model, opt, infos


def _dynamics(model, loss_fn, n_steps, dt, precond):
    import time
    from hidenn_fem_amd.dynamics import NewmarkSolver
    from hidenn_fem_amd.modal import vibration_modes
    if dt is None:
        lam = vibration_modes(model, loss_fn, n_modes=1, precond=precond, max_iter=200 if precond == "amg" else 5000).eigenvalues[0].item()
        dt = 2.0 * 3.141592653589793 / lam ** 0.5 / 20.0
        print(f"lowest mode: period {20.0 * dt:.6e}; dt = period / 20 = {dt:.6e}")
    with torch.no_grad():
        model.u_free.zero_()
    solver = NewmarkSolver(model, loss_fn, dt, precond=precond)
    solver.set_state()
    x = model.coords.detach()[model._idx_ufree.to(model.coords.device)]                 # node of every free u row (storage order)
    tip = int(torch.argmax(x[:, 0] - 1e-3 * (x[:, 1] - 0.5 * x[:, 1].max()).abs()))     # right edge, nearest mid-height
    print(f"step load from rest (consistent mass, density 1, beta 1/4, gamma 1/2, {precond}); tip = free row {tip} at "
          f"({x[tip, 0].item():.3f}, {x[tip, 1].item():.3f})")
    infos = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        info = solver.step(1)[0]
        u = solver.u[tip]
        print(f"t {info.t:.6e}: tip u ({u[0].item():+.6e}, {u[1].item():+.6e}) CG {info.iterations:4d} ({info.reason}) "
              f"energy {solver.energy()['total']:+.9e}")
        infos.append(info)
    torch.cuda.synchronize()
    print(f"{n_steps} steps, {sum(i.iterations for i in infos)} CG iterations, {time.perf_counter() - t0:.3f} s")
    return model, infos


def _hyper_dynamics(model, loss_fn, lin_loss, t_force, n_steps, dt, precond):
    import time
    from hidenn_fem_amd.dynamics import HyperNewmarkSolver
    from hidenn_fem_amd.modal import vibration_modes
    if dt is None:
        lam = vibration_modes(model, lin_loss, n_modes=1, precond=precond, max_iter=200 if precond == "amg" else 5000).eigenvalues[0].item()
        dt = 2.0 * 3.141592653589793 / lam ** 0.5 / 20.0
        print(f"lowest mode of the linearised plate: period {20.0 * dt:.6e}; dt = period / 20 = {dt:.6e}")
    with torch.no_grad():
        model.u_free.zero_()
    solver = HyperNewmarkSolver(model, loss_fn, dt, precond=precond, t_force=t_force)
    solver.set_state()
    x = model.coords.detach()[model._idx_ufree.to(model.coords.device)]                 # node of every free u row (storage order)
    tip = int(torch.argmax(x[:, 0] - 1e-3 * (x[:, 1] - 0.5 * x[:, 1].max()).abs()))     # right edge, nearest mid-height
    print(f"step load from rest at finite strain (consistent mass, density 1, beta 1/4, gamma 1/2, {precond}); tip = free row "
          f"{tip} at ({x[tip, 0].item():.3f}, {x[tip, 1].item():.3f})")
    infos = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        info = solver.step(1)[0]
        infos.append(info)
        if info.reason in ("inverted", "line_search"):
            print(f"t {info.t:.6e}: the step stopped with {info.reason!r}; the state is the one before it")
            break
        u = solver.u[tip]
        print(f"t {info.t:.6e}: tip u ({u[0].item():+.6e}, {u[1].item():+.6e}) Newton {info.newton_iterations:2d} CG "
              f"{info.iterations:5d} ({info.reason}) min J {info.min_J:.4f} energy {solver.energy()['total']:+.9e}")
    torch.cuda.synchronize()
    print(f"{len(infos)} steps, {sum(i.newton_iterations for i in infos)} Newton and {sum(i.iterations for i in infos)} CG "
          f"iterations, {time.perf_counter() - t0:.3f} s")
    return model, infos


def _print_error(model, loss_fn, when, recovery=None):
    """One line with the relative ZZ error estimate; returns the ``StressRecovery`` (reusable: the connectivity never changes)."""
    from hidenn_fem_amd.post import StressRecovery
    recovery = recovery or StressRecovery(model, loss_fn)
    err = recovery.error()
    print(f"ZZ error estimate {when}: eta_rel {err.relative:.6e} (eta {err.eta:.6e}, ||u_h|| {err.energy_norm2 ** 0.5:.6e}, "
          f"largest element share {(err.eta2.max().item() / max(err.eta ** 2, 1e-300)):.3e})")
    return recovery


def _r_adapt(model, loss_fn, outer, precond="block_jacobi", error_estimate=False):
    import time
    from hidenn_fem_amd.radapt import mesh_quality, quad4_mesh_quality, r_adapt_
    quality = quad4_mesh_quality if getattr(model, "nodes_per_element", 3) == 4 else mesh_quality
    recovery = None
    if error_estimate:                    # the frozen-mesh state r_adapt_ starts from: the same solve, made once more there
        from hidenn_fem_amd.solve import solve_displacement_
        solve_displacement_(model, loss_fn, rtol=1e-10, precond=precond)
        recovery = _print_error(model, loss_fn, "on the frozen mesh")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = r_adapt_(model, loss_fn, max_outer=outer, cg_precond=precond)      # RAdaptiveSolver / Quad4RAdaptiveSolver
    torch.cuda.synchronize()
    print(f"frozen-mesh energy {info.energy[0]:.9e} ({info.cg_iterations[0]} CG iterations)")
    for k in range(1, info.iterations + 1):
        print(f"outer {k:3d}: energy {info.energy[k]:.9e} |g_x|inf {info.grad_inf[k]:.3e} alpha {info.alpha[k]:.3e} "
              f"(max {info.alpha_max[k]:.3e}) CG {info.cg_iterations[k]} min q {info.min_q[k]:.4f}")
    mq = quality(model)
    print(f"r-adapted energy {info.energy[-1]:.9e} after {info.iterations} outer iterations ({info.reason}), "
          f"min q {mq.min_q:.4f}, inverted elements {mq.n_inverted}, {time.perf_counter() - t0:.3f} s")
    if error_estimate:
        _print_error(model, loss_fn, "on the r-adapted mesh", recovery)
    return model, info.energy[-1]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=200)
    ap.add_argument("--ny", type=int, default=100)
    ap.add_argument("--steps", type=int, default=None, help="outer L-BFGS steps (default 30; per load increment of --neo-hookean: 100)")
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--fused-lbfgs", action="store_true")
    ap.add_argument("--sharded", action="store_true", help="owner-sharded energy + node-sharded L-BFGS (one process per GPU)")
    ap.add_argument("--solve-first", action="store_true", help="start L-BFGS from the frozen-mesh displacement solve (CG)")
    ap.add_argument("--r-adapt", action="store_true",
                    help="alternating r-adaptive solve (frozen-mesh CG, inversion-safe coordinate steps) instead of L-BFGS; "
                         "with --neo-hookean: the finite-strain one at the full load (Newton-Krylov, det F-safe steps)")
    ap.add_argument("--outer", type=int, default=None, help="outer iterations of --r-adapt (default 20; with --neo-hookean: 10)")
    ap.add_argument("--quad", action="store_true",
                    help="with --r-adapt or --neo-hookean: the plate as nx x ny nodes of QUAD4 cells (no holes)")
    ap.add_argument("--precond", choices=["block_jacobi", "amg", "amg_tangent"], default="block_jacobi",
                    help="CG preconditioner of --solve-first, --r-adapt and --neo-hookean --newton (amg_tangent: the latter only)")
    ap.add_argument("--error-estimate", action="store_true",
                    help="print the relative ZZ error estimate after the solve (with --r-adapt: before and after adaptation); "
                         "builds the loss with grad_convention='physical'.  With --neo-hookean: the finite-strain indicator on "
                         "the recovered Cauchy stress after every load increment (and before and after --r-adapt)")
    ap.add_argument("--neo-hookean", action="store_true",
                    help="the plate at finite strain: Neo-Hookean material, load ramped in steps, FusedLBFGS on u_free (fp64)")
    ap.add_argument("--load-steps", type=int, default=8, help="load increments of --neo-hookean")
    ap.add_argument("--modes", type=int, default=0, metavar="N",
                    help="print the N lowest free-vibration frequencies of the plate (block LOBPCG, N <= 8; with --quad and "
                         "--precond block_jacobi|amg) and stop")
    ap.add_argument("--dynamics", type=int, default=0, metavar="N",
                    help="a step load on the plate at rest, N Newmark steps (t, tip displacement, CG iterations and total "
                         "energy per step; with --dt, --quad and --precond block_jacobi|amg) and stop; with --neo-hookean: at "
                         "finite strain (a Newton-Krylov solve per step; also Newton iterations and min J)")
    ap.add_argument("--dt", type=float, default=None, help="time step of --dynamics (default: 1/20 of the lowest mode's period)")
    ap.add_argument("--buckling", type=int, default=0, metavar="N",
                    help="reverse the default traction into compression, solve, print the N smallest buckling load factors and "
                         "the critical load (block LOBPCG, N <= 8; with --quad and --precond block_jacobi|amg) and stop")
    ap.add_argument("--harmonic", type=int, default=0, metavar="N",
                    help="the tip amplitude of the steady-state response to the default traction at N frequencies spanning the "
                         "first three modes, 2 %% Rayleigh damping (COCG; with --quad and --precond block_jacobi|amg) and stop")
    ap.add_argument("--topopt", type=int, default=0, metavar="N",
                    help="N design iterations of SIMP compliance topology optimisation under the default traction (volume "
                         "fraction 0.4, OC update; with --quad and --precond block_jacobi|amg) and stop")
    ap.add_argument("--plasticity", type=int, default=0, metavar="N",
                    help="the plate as a J2 elastoplastic load path: the default traction ramped up in N steps and back down in N "
                         "(plastic fraction and max alpha per step; with --precond block_jacobi|amg) and stop")
    ap.add_argument("--newton", action="store_true",
                    help="with --neo-hookean: solve every load increment with NewtonKrylovSolver (with --quad: "
                         "Quad4NewtonKrylovSolver) instead of FusedLBFGS")
    a = ap.parse_args()
    if a.precond == "amg_tangent" and not (a.neo_hookean and (a.newton or a.r_adapt)):
        ap.error("--precond amg_tangent needs --neo-hookean with --newton or --r-adapt (with or without --quad)")
    if a.harmonic and a.neo_hookean:
        ap.error("--harmonic is a linear analysis: drop --neo-hookean")
    if a.topopt and a.neo_hookean:
        ap.error("--topopt is a linear analysis: drop --neo-hookean")
    if a.plasticity:
        if a.neo_hookean or a.quad or a.precond == "amg_tangent":
            ap.error("--plasticity runs on triangles at small strain with --precond block_jacobi|amg: drop --neo-hookean / --quad")
        run_plasticity(a.nx, a.ny, a.plasticity, precond=a.precond)
        raise SystemExit(0)
    if a.neo_hookean:
        run_neo_hookean(a.nx, a.ny, a.steps or 100, load_steps=a.load_steps, newton=a.newton, precond=a.precond, quad=a.quad,
                        dynamics=a.dynamics, dt=a.dt,
                        r_adapt=a.r_adapt, outer=a.outer or 10, error_estimate=a.error_estimate)
        raise SystemExit(0)
    run(a.nx, a.ny, a.steps or 30, torch.float64 if a.fp64 else torch.float32, fused_lbfgs=a.fused_lbfgs, sharded=a.sharded,
        solve_first=a.solve_first, r_adapt=a.r_adapt, outer=a.outer or 20,
        precond=a.precond, quad=a.quad, error_estimate=a.error_estimate, modes=a.modes, dynamics=a.dynamics, dt=a.dt,
        buckling=a.buckling, harmonic=a.harmonic, topopt=a.topopt)
