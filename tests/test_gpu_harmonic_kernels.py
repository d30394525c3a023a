"""The complex shifted apply of the harmonic solver (csrc/harmonic.hip) and its unconjugated ``p^T A p`` against the
sparse reference ``z_K K + z_M M`` -- K from ``assemble_stiffness``, M from tests/modal_reference.py with rho = 2, both as
tests/test_gpu_dynamics_kernels.py holds them (its shape tables, model builders and ``_mass`` are imported, not copied): every
TRI3 and QUAD4 tile shape of the dispatch whose tiles fit the 64 KiB LDS rule, both gradient conventions, consistent and lumped
mass; a shape that does not fit is refused with the documented message.  Then the smallest cases, and the halting contract.

Tolerances: apply 1e-12 x max |q| (what the project holds for the shifted apply); ``p^T A p`` per component
1e-12 x (|z_K| p^H K p + |z_M| p^H M p): a bound on the terms, not on the possibly cancelling sum."""
import numpy as np
import pytest
import torch

import test_gpu_dynamics_kernels as DK

pytestmark = pytest.mark.gpu
F64 = torch.float64
RHO = DK.RHO
OMEGA2 = 3.7                                                 # the (1, -omega^2 rho) case: z_M = -OMEGA2 (times rho inside)
# (z_K, z_M): the operator is z_K K + z_M rho M
COEFFS = {"K": (1.0, 0.0), "M": (0.0, 1.0), "real": (1.0, -OMEGA2), "iK": (1.0j, 0.0), "general": (0.3 + 0.7j, -1.7 + 0.2j)}
LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cases cached by tests/test_gpu_dynamics_kernels.py own library handles: let them go with this module too."""
    yield
    DK._case.cache_clear()


def lds_need(stats):
    """The documented rule (include/hidenn_fem.h): 48 per local node + 32 per owned row + 8 (2 threads / 64 + 2)."""
    return 48 * stats["max_tile_nodes"] + 32 * stats["max_tile_owned"] + 8 * (2 * (stats["threads_per_tile"] // 64) + 2)


def _solver(m, lf, mass, **kw):
    from hidenn_fem_amd.harmonic import HarmonicSolver
    kw.setdefault("precond", "block_jacobi")
    return HarmonicSolver(m, lf, density=RHO, mass=mass, **kw)


def _refused(m, lf, plan):
    need = lds_need(plan.stats)
    with pytest.raises(ValueError, match="tile_elems") as e:
        _solver(m, lf, "consistent")
    msg = str(e.value)
    assert "more than 64 KiB of LDS" in msg and f"48 x {plan.stats['max_tile_nodes']} local nodes" in msg
    assert f"32 x {plan.stats['max_tile_owned']} owned rows" in msg and f"= {need} bytes > 65536" in msg


def _check_apply(s, K, M, p, what):
    n = s.n_u
    pn = p.cpu().numpy().reshape(-1)
    pr, pi = np.ascontiguousarray(pn.real), np.ascontiguousarray(pn.imag)
    pKp = pr @ (K @ pr) + pi @ (K @ pi)
    pMp = pr @ (M @ pr) + pi @ (M @ pi)
    dev = p.device
    plain = [s.solver.apply(torch.as_tensor(v.reshape(n, 2), dtype=F64, device=dev))[0].cpu().numpy().reshape(-1) for v in (pr, pi)]
    for name, (zk, zm) in COEFFS.items():
        pv, p_t = pn, p
        if name == "real":
            pv, p_t = pr.astype(complex), p.real.contiguous()
        want = zk * (K @ pv) + zm * (M @ pv)
        q, pq = s.operator_apply(p_t, coefficients=(zk, zm))
        assert q.dtype == torch.complex128 and tuple(q.shape) == (n, 2) and pq.dtype == torch.complex128
        qn = q.cpu().numpy().reshape(-1)
        scale = np.abs(want).max()
        err = np.abs(qn - want).max() / scale
        pq_ref = pv @ want                                   # unconjugated
        term = abs(zk) * (pKp if name != "real" else pr @ (K @ pr)) + abs(zm) * (pMp if name != "real" else pr @ (M @ pr))
        d = pq.item() - pq_ref
        print(f"{what} {name}: apply {err:.2e}  p^T A p re {abs(d.real) / term:.2e} im {abs(d.imag) / term:.2e}")
        assert err <= 1e-12, (what, name, err)
        assert abs(d.real) <= 1e-12 * term and abs(d.imag) <= 1e-12 * term, (what, name, d, term)
        if name == "K":                                      # each plane is the plain hfem_cg_apply of that plane
            for got, ref in ((qn.real, plain[0]), (qn.imag, plain[1])):
                assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (what, name)
        if name == "real":                                   # real coefficients, real p: nothing reaches the imaginary plane
            assert not qn.imag.any(), (what, np.abs(qn.imag).max())
        if name == "iK":                                     # i K (p_r + i p_i) = -K p_i + i K p_r
            assert np.abs(qn.real + plain[1]).max() <= 1e-12 * np.abs(plain[1]).max(), what
            assert np.abs(qn.imag - plain[0]).max() <= 1e-12 * np.abs(plain[0]).max(), what


def _complex_p(n, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(n, 2, dtype=F64, generator=g), torch.randn(n, 2, dtype=F64, generator=g)).to(dev)


@pytest.mark.parametrize("conv", DK.CONVS)
@pytest.mark.parametrize("mass", ["consistent", "lumped"])
@pytest.mark.parametrize("kind,shape", DK.ALL_SHAPES, ids=[f"{k}-{s}" for k, s in DK.ALL_SHAPES])
def test_complex_apply_against_the_sparse_operator(kind, shape, mass, conv):
    m, lf, plan, K, Ms = DK._case(kind, shape, conv)
    if lds_need(plan.stats) > LDS_LIMIT:                     # computed from plan.stats: this shape's tiles do not fit
        _refused(m, lf, plan)
        return
    s = _solver(m, lf, mass)
    assert s.solver.plan is plan                             # the branch asserted on `plan` is the one that runs
    _check_apply(s, K, Ms[mass == "lumped"], _complex_p(s.n_u, DK._dev()), f"{kind}-{shape} {mass} {conv}")


def test_a_plan_whose_tiles_exceed_64_kib_is_refused_with_the_numbers():
    """At least one refused plan: a listed shape where one exceeds the limit, else the structured 101 x 51 TRI3 mesh with
    ``tile_elems`` raised until a tile does (1024 local nodes take 48 KiB, 510 owned rows the rest)."""
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.plan import model_plan
    for kind, shape in DK.ALL_SHAPES:
        m, lf, plan, _, _ = DK._case(kind, shape, "physical")
        if lds_need(plan.stats) > LDS_LIMIT:
            _refused(m, lf, plan)
            return
    m = DK._case("tri3", "c", "physical")[0]
    tried = []
    for te in range(1500, 2101, 100):
        try:
            plan = model_plan(m, te, paired=True)
        except RuntimeError as e:                            # the planner could not fit a tile into 1024 local nodes
            tried.append((te, str(e)[:60]))
            continue
        tried.append((te, plan.stats["max_tile_nodes"], plan.stats["max_tile_owned"], lds_need(plan.stats)))
        if plan.stats["paired"] and lds_need(plan.stats) > LDS_LIMIT:
            _refused(m, EnergyLoss2D(device=DK._dev(), dtype=F64, tile_elems=te, grad_convention="physical"), plan)
            return
    pytest.fail(f"no plan exceeded the limit: {tried}")


@pytest.mark.parametrize("conv", DK.CONVS)
def test_quad4_four_per_thread_instance_on_a_tile_that_fits(conv):
    """The listed QUAD4 shape of the <4,4> instance (tile_elems 800) exceeds the LDS rule, so the instance is reached here on
    the same mesh with the largest tiles that fit: tile_elems 700 gives 845 local nodes and 784 slots (the fourth node and slot
    of a thread both populated) at 65152 bytes."""
    import test_gpu_quad4_shapes as QS
    from hidenn_fem_amd.solve import assemble_stiffness
    m = QS._new_model("S", DK._dev(), conv=conv)
    tried = []
    for te in (700, 690, 680):
        plan = m.tile_plan(te)
        tried.append((te, QS.quad4_cg_apply_branch(plan.stats), lds_need(plan.stats)))
        if tried[-1][1] == "<4,4>" and tried[-1][2] <= LDS_LIMIT:
            lf = QS._lf(tile_elems=te)
            K = DK._scipy(assemble_stiffness(m, lf))
            s = _solver(m, lf, "consistent")
            assert s.solver.plan is plan
            _check_apply(s, (0.5 * (K + K.T)).tocsr(), DK._mass(m, False), _complex_p(s.n_u, DK._dev()), f"quad4 S te={te} {conv}")
            return
    pytest.fail(f"no <4,4> tile plan fits the LDS rule: {tried}")


def _single_cell(kind, conv):
    """One clamped cell: 2 triangles / 1 quad, left edge clamped, two free nodes."""
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    from hidenn_fem_amd.solve import assemble_stiffness
    gen, cls = (structured_quad_mesh, QuadShapeNN2D) if kind == "quad4" else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, _, edges = gen(2, 2, length=1.3, height=0.9, dtype=F64)
    # every node of one cell is a boundary node: the coordinate rows are kept free here (no boundary mask), the solvers bind
    # free coordinate rows
    m = cls(nc, conn, boundary_mask=torch.zeros_like(geom), dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(DK._dev())
    lf = EnergyLoss2D(device=DK._dev(), dtype=F64, grad_convention=conv)
    assert int(m.u_free.shape[0]) == 2 and m.Nelems == (1 if kind == "quad4" else 2)
    K = DK._scipy(assemble_stiffness(m, lf))
    return m, lf, (0.5 * (K + K.T)).tocsr()


@pytest.mark.parametrize("conv", DK.CONVS)
@pytest.mark.parametrize("mass", ["consistent", "lumped"])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_complex_apply_on_a_single_clamped_cell(kind, mass, conv):
    m, lf, K = _single_cell(kind, conv)
    s = _solver(m, lf, mass)
    assert s.n_u == 2 and s.solver.plan.stats["n_tiles"] == 1
    _check_apply(s, K, DK._mass(m, mass == "lumped"), _complex_p(2, DK._dev(), seed=9), f"{kind} cell {mass} {conv}")


@pytest.mark.parametrize("precond", ["none", "block_jacobi", "amg"])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_after_a_halt_further_iterations_leave_x_bit_identical(kind, precond):
    """Converged, stopped by max_iter, and broken down (b isotropic in the unconjugated form: rho = b^T b = 0 on the first
    direction, so x never moves): every later launch returns at once."""
    m, lf, plan, K, Ms = DK._case(kind, "a" if kind == "tri3" else "S600", "physical")
    s = _solver(m, lf, "consistent", precond=precond, rayleigh=(0.3, 1e-7), rtol=1e-9)
    # inside the spectrum of the pencil (the Rayleigh quotient of the diagonals bounds lambda_max from below): A is
    # indefinite and far from the preconditioner's K + omega^2 M, so two iterations cannot meet 1e-9
    omega = 0.5 * float(np.sqrt(K.diagonal().mean() / Ms[False].diagonal().mean()))
    for cap, b, want in ((None, None, ("rtol",)), (2, None, ("max_iter",)), (None, "isotropic", ("breakdown",))):
        s.max_iter = max(1000, 4 * s.n_u) if cap is None else cap
        rhs = None
        if b == "isotropic":
            if precond != "none":
                continue                                     # T b need not be isotropic: the case is for the plain form
            v = torch.zeros(s.n_u, 2, dtype=torch.complex128, device=DK._dev())
            v[0, 0], v[0, 1] = 1.0, 1.0j
            rhs = v
        u, info = s.solve(omega, b=rhs)
        assert info.reason in want, (kind, precond, info)
        st0 = s._read_status()
        x0 = s._x.clone()
        for _ in range(2):
            s._iterate()                                     # eager launches
            s._replay()                                      # and the captured graph
        st1 = s._read_status()
        assert torch.equal(s._x, x0) and st1 == st0, (kind, precond, info)
        if want == ("breakdown",):
            assert info.iterations == 0 and not s._x.any()
        if want == ("max_iter",):
            assert info.iterations == 2 and not info.converged
    s.max_iter = max(1000, 4 * s.n_u)
