"""The PCG recursion and the stopping rule of the frozen-mesh solve (csrc/cg.hip; element kernels csrc/tri3_cg.hip,
csrc/quad4_cg.hip), step by step:
every slot of the status record and ``u`` after every iteration against ``cg_reference.pcg_steps`` in longdouble on an
operator that does not come from the code under test (the dense oracle Hessian; for AMG the assembled K_ff, which
test_gpu_amg.py holds to the oracle, and the reference V-cycle on the arrays read back from the device), the recursion's |r|
against the true residual, and every outcome of the stopping rule with thresholds taken from the reference's |r_k| sequence.

Tolerances are measured, not fixed: the float64 run of the reference deviates ``dev_k`` from its longdouble run up to step k,
and the kernel may deviate ``cg_reference.allowed(dev_k)`` = 32 dev_k + 64 eps from the longdouble run."""
import math

import numpy as np
import pytest
import torch

import cg_reference as R
from test_gpu_amg_cycle import _storage_order, device_levels
from test_gpu_solve import _dev_forces, _golden_model, _loss, _oracle, _structured
from test_gpu_solve_quad4 import BASE, _lf, _model as _quad_model, _oracle as _quad_oracle

pytestmark = pytest.mark.gpu
F64 = torch.float64
LD = np.longdouble
DEV = torch.device("cuda:0")
TRI_CASE = "permuted_random_diag"          # the largest golden case with Dirichlet rows and a body force: 99 free rows
# the stopping tests need a first k in 4..8 whose |r_k| is 1.44 below every earlier one: from the golden starts (random
# u_free, |r_0| ~ 30 |f|) block Jacobi's |r| is not monotone on most cases; this one has k = 4 (56 free rows)
STOP_TRI_CASE = "no_boundary_mask"
NO_STOP = dict(rtol=0.0, atol=0.0, max_iter=10 ** 6)


def _make(kind, conv, precond, g_tri, tri_case=TRI_CASE, **kw):
    """(solver, dense or block-sparse K in storage order that the solver did not produce)."""
    from hidenn_fem_amd.solve import FrozenMeshSolver, Quad4FrozenMeshSolver, assemble_stiffness
    if kind == "tri3":
        H, _, _ = _oracle(g_tri, tri_case, conv)
        m = _golden_model(g_tri, tri_case, conv=conv)
        lf, _, _ = _loss(g_tri, tri_case)
        _, _, bd, td = _dev_forces(tri_case)
        return FrozenMeshSolver(m, lf, b_force=bd, t_force=td, precond=precond, **kw), _storage_order(m, H).numpy()
    if kind == "quad4":
        H, _, _ = _quad_oracle(conv)
        m = _quad_model(conv=conv, **BASE)
        return Quad4FrozenMeshSolver(m, _lf(), precond=precond, **kw), _storage_order(m, H).numpy()
    assert kind == "tri3_amg" and precond == "amg"
    m = _structured("auto", nx=121, ny=61)
    m.grad_convention = conv
    lf = _lf()
    K = assemble_stiffness(m, lf)
    n = m.u_free.shape[0]
    Kb = R.Bsr(K.values().cpu().numpy(), K.crow_indices().cpu().numpy(), K.col_indices().cpu().numpy(), 2, 2, n)
    return FrozenMeshSolver(m, lf, precond="amg", **kw), Kb


def _cast(K, dtype):
    return K.astype(dtype)


def _precond(s, dtype):
    """M of the solver after its refresh, restated in ``dtype``."""
    if s.precond == "none":
        return None
    if s.precond == "block_jacobi":
        return R.block_jacobi(s.diag.cpu().numpy(), dtype)
    levels, coarse_inv = device_levels(s)
    lv = R.cast_levels(levels, dtype)
    assert len(lv) >= 2                                              # a real hierarchy: three levels
    return lambda r: R.vcycle(lv, coarse_inv, r, dtype)


def _prime(s, rtol, atol, max_iter):
    """What ``solve()`` does up to and including ``_start``; the status record of iteration 0."""
    s.refresh()
    with torch.no_grad():
        s._u.copy_(s.model.u_free.detach())
        s._gradient(s._u, s._g0)
        s._gradient(s._zero, s._gz)
        s._start(rtol, atol, max_iter)
    return s._read_status()


def _restart(s, rtol, atol, max_iter):
    """``_start`` again on the gradients already in place: |f| is reduced in a fixed order, so it repeats to the bit."""
    s._start(rtol, atol, max_iter)
    return s._read_status()


def _drive(s, max_iter):
    """The loop of ``solve()`` after ``_start``."""
    st = s._read_status()
    while not st[R.ST_HALTED] and st[R.ST_ITER] < max_iter:
        s._replay()
        st = s._read_status()
    return st


def _reference(s, K, n):
    """``pcg_steps`` in longdouble and in float64 from the primed solver's own g0, gz and u, their per-step deviation, and
    the float64 run's drift: the gap between its recursive |r| and the true |f - K u| (longdouble), over |r_0|, up to step k."""
    R.assert_longdouble_is_wider()
    g0, gz, u0 = (t.cpu().numpy().reshape(-1) for t in (s._g0, s._gz, s._u))
    Kh = _cast(K, LD)
    hi = R.pcg_steps(Kh, _precond(s, LD), g0, gz, n, LD, u0=u0)
    lo = R.pcg_steps(_cast(K, np.float64), _precond(s, np.float64), g0, gz, n, np.float64, u0=u0)
    dev = R.pcg_deviation(lo, hi)
    f = -gz.astype(LD)
    drift, run = [], 0.0
    for rec in lo:
        run = max(run, float(abs(_true_rnorm(Kh, f, rec["u"]) - LD(rec["rnorm"])) / hi[0]["rnorm"]))
        drift.append(run)
    return dict(hi=hi, lo=lo, dev=dev, drift=drift, K=Kh, f=f, fnorm_dev=float(abs(LD(lo[0]["fnorm"]) - hi[0]["fnorm"]) / hi[0]["fnorm"]))


def _true_rnorm(Kh, f, u):
    r = f - R._apply(Kh, np.asarray(u, dtype=LD).reshape(-1))
    return np.sqrt(r @ r)


def _relerr(got, want):
    return float(abs(LD(got) - want) / abs(want)) if want != 0 else float(abs(got))


# ---------------------------------------------------------------- the recursion
PARAMS = [(k, c, p) for k in ("tri3", "quad4") for c in ("reference", "physical") for p in ("none", "block_jacobi")] + \
         [("tri3_amg", c, "amg") for c in ("reference", "physical")]


@pytest.mark.parametrize("kind,conv,precond", PARAMS)
def test_every_iteration_matches_the_reference_recursion(g_tri, kind, conv, precond):
    """12 iterations (6 with AMG), the first half through ``_iterate`` (plain launches), the second through ``_replay`` (the
    captured graph), ``iters_per_graph=1``.  After each: kIter exactly; kAlpha, kPq, kRho, kBeta, kRnorm and ``_u`` within
    ``allowed(dev_k)`` of the longdouble recursion; kRnorm within ``allowed(drift_k)`` |r_0| of the true |f - K u| formed in
    longdouble from the device's ``_u`` (drift_k: the same gap in the float64 reference run -- the recursion's own drift)."""
    n = 6 if precond == "amg" else 12
    s, K = _make(kind, conv, precond, g_tri, iters_per_graph=1, **NO_STOP)
    st = _prime(s, **NO_STOP)
    ref = _reference(s, K, n)
    hi, dev, drift = ref["hi"], ref["dev"], ref["drift"]
    # the record of iteration 0
    assert st[R.ST_ITER] == 0.0 and st[R.ST_HALTED] == 0.0 and st[R.ST_REASON] == 0.0
    assert st[R.ST_TOL] == 0.0 and st[R.ST_MAXITER] == float(NO_STOP["max_iter"]) and st[R.ST_RTOLWINS] == 1.0
    assert st[R.ST_ALPHA] == 0.0 and st[R.ST_BETA] == 0.0 and st[R.ST_PQ] == 0.0
    assert _relerr(st[R.ST_FNORM], hi[0]["fnorm"]) <= R.allowed(ref["fnorm_dev"])
    assert _relerr(st[R.ST_RNORM], hi[0]["rnorm"]) <= R.allowed(dev[0]["rnorm"])
    assert _relerr(st[R.ST_RHO], hi[0]["rho"]) <= R.allowed(dev[0]["rho"])
    worst = {q: (0.0, 0.0) for q in R.SCALARS + ("u", "drift")}
    slots = dict(alpha=R.ST_ALPHA, pq=R.ST_PQ, rho=R.ST_RHO, beta=R.ST_BETA, rnorm=R.ST_RNORM)
    for k in range(1, n + 1):
        if k <= n // 2:
            s._iterate()
        else:
            s._replay()
        st = s._read_status()
        u = s._u.cpu().numpy().reshape(-1)
        assert st[R.ST_ITER] == float(k) and st[R.ST_HALTED] == 0.0, (k, st)
        got = {q: _relerr(st[slot], hi[k][q]) for q, slot in slots.items()}
        got["u"] = R.rel(u, hi[k]["u"])
        got["drift"] = float(abs(_true_rnorm(ref["K"], ref["f"], u) - LD(st[R.ST_RNORM])) / hi[0]["rnorm"])
        want = dict(dev[k], drift=drift[k])
        print(f"step {k:2d} ({kind}, {conv}, {precond}): " +
              ", ".join(f"{q} {got[q]:.2e} (ref {want[q]:.2e})" for q in got))
        for q in got:
            worst[q] = max(worst[q], (got[q], want[q]))
            assert got[q] <= R.allowed(want[q]), (k, q, got[q], want[q], R.allowed(want[q]))
    print(f"largest ({kind}, {conv}, {precond}): " + ", ".join(f"{q} kernel {v[0]:.2e} ref {dev[n].get(q, drift[n]):.2e}"
                                                               for q, v in worst.items()))


@pytest.mark.parametrize("kind,conv,precond", [p for p in PARAMS if p[1] == "reference" and p[2] != "none"])
def test_start_record_holds_the_tolerance_and_who_wins(g_tri, kind, conv, precond):
    """kTol = max(rtol |f|, atol), kMaxIter and kRtolWins (rtol |f| >= atol) after ``_start``, for tolerances that do not halt."""
    s, _ = _make(kind, conv, precond, g_tri, iters_per_graph=1)
    fn = _prime(s, 0.0, 0.0, 7)[R.ST_FNORM]
    assert fn > 0.0
    for rtol, atol, wins in ((1e-9, 1e-30, 1.0), (1e-12, 1e-9 * fn, 0.0), (0.0, 1e-9 * fn, 0.0), (1e-9, 0.0, 1.0)):
        st = _restart(s, rtol, atol, 7)
        assert st[R.ST_FNORM] == fn                                  # |f| is reduced in a fixed order
        assert st[R.ST_TOL] == max(rtol * fn, atol) and st[R.ST_MAXITER] == 7.0 and st[R.ST_RTOLWINS] == wins, (rtol, atol, st)
        assert st[R.ST_HALTED] == 0.0 and st[R.ST_ITER] == 0.0


@pytest.mark.parametrize("kind,conv,precond", [p for p in PARAMS if p[2] != "none"])
def test_solve_info_reports_the_recursions_residual_and_the_rhs_norm(g_tri, kind, conv, precond):
    """``SolveInfo.rhs_norm`` against |gz| in longdouble; ``SolveInfo.residual_norm`` against the true |f - K u| of the
    returned ``u_free``, within the drift the float64 reference shows over as many iterations (sampled, and at the last)."""
    s, K = _make(kind, conv, precond, g_tri, rtol=1e-10, iters_per_graph=16)
    info = s.solve()
    assert info.converged and info.reason == "rtol" and 0 < info.iterations < 2000, info
    ref = _reference_from_solved(s, K, info.iterations)
    assert _relerr(info.rhs_norm, ref["fnorm"]) <= R.allowed(ref["fnorm_dev"]), (info, ref["fnorm"])
    u = s.model.u_free.detach().cpu().numpy().reshape(-1)
    true = _true_rnorm(ref["K"], ref["f"], u)
    gap = float(abs(true - LD(info.residual_norm)) / ref["r0"])
    print(f"solve ({kind}, {conv}, {precond}): {info}; true |f - K u| {float(true):.6e}; gap / |r_0| {gap:.2e} (ref drift "
          f"{ref['drift']:.2e}); rhs_norm err {_relerr(info.rhs_norm, ref['fnorm']):.2e} (ref {ref['fnorm_dev']:.2e})")
    assert info.residual_norm <= 1e-10 * info.rhs_norm
    assert gap <= R.allowed(ref["drift"]), (gap, ref["drift"])


def _reference_from_solved(s, K, n):
    """The float64 reference run over ``n`` iterations from the g0 / gz that ``solve()`` left in the solver.  It starts from
    u = 0, so its ``u`` is the increment u_k - u_0 and its true residual is r_0 - K (u_k - u_0) with r_0 = -g0."""
    g0, gz = (t.cpu().numpy().reshape(-1) for t in (s._g0, s._gz))
    Kh = _cast(K, LD)
    f = -gz.astype(LD)
    lo = R.pcg_steps(_cast(K, np.float64), _precond(s, np.float64), g0, gz, n, np.float64)
    r0v = -g0.astype(LD)
    r0 = np.sqrt(r0v @ r0v)
    drift = 0.0
    for k in sorted(set(range(0, n + 1, max(1, n // 16))) | {n}):
        r = r0v - R._apply(Kh, lo[k]["u"].astype(LD))
        drift = max(drift, float(abs(np.sqrt(r @ r) - LD(lo[k]["rnorm"])) / r0))
    fn = np.sqrt(f @ f)
    return dict(K=Kh, f=f, r0=r0, drift=drift, fnorm=fn, fnorm_dev=float(abs(LD(lo[0]["fnorm"]) - fn) / fn))


# ---------------------------------------------------------------- the stopping rule
_STOP_REF = {}


def _stop_reference(g_tri, kind):
    """The longdouble |r_k| sequence and iterates of the block-Jacobi solve of ``kind`` (reference convention), once."""
    if kind not in _STOP_REF:
        s, K = _make(kind, "reference", "block_jacobi", g_tri, tri_case=STOP_TRI_CASE, iters_per_graph=1)
        _prime(s, **NO_STOP)
        _STOP_REF[kind] = _reference(s, K, 12)
    return _STOP_REF[kind]


def _threshold(rn):
    """(k, t): the first k in 4..8 with |r_k| <= t, every |r_i|, i <= k, a factor 1.2 or more away from t."""
    for k in range(4, 9):
        prev = min(rn[:k])
        if rn[k] * 1.44 <= prev:
            return k, math.sqrt(rn[k] * prev)
    return None


def _halted_for_good(s):
    st0, u0 = s._read_status(), s._u.clone()
    assert st0[R.ST_HALTED] == 1.0
    for _ in range(3):
        s._replay()
    assert s._read_status() == st0 and torch.equal(s._u, u0)


def _run(g_tri, kind, ipg, precond="block_jacobi", **kw):
    s, _ = _make(kind, "reference", precond, g_tri, tri_case=STOP_TRI_CASE, iters_per_graph=ipg, **kw)
    u0 = s.model.u_free.detach().clone()
    info = s.solve()
    _halted_for_good(s)
    return s, info, u0


def _assert_iterate(s, ref, k):
    got = R.rel(s.model.u_free.detach().cpu().numpy().reshape(-1), ref["hi"][k]["u"])
    assert got <= R.allowed(ref["dev"][k]["u"]), (k, got, ref["dev"][k]["u"])


@pytest.mark.parametrize("ipg", [1, 16])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_atol_rtol_and_their_tie_stop_at_the_iteration_the_reference_names(g_tri, kind, ipg):
    ref = _stop_reference(g_tri, kind)
    rn = [float(r["rnorm"]) for r in ref["hi"]]
    fn = float(ref["hi"][0]["fnorm"])
    found = _threshold(rn)
    assert found is not None, rn
    k, t = found
    assert all(r >= 1.2 * t for r in rn[:k]) and rn[k] * 1.2 <= t
    cases = {"atol": (0.0, t, "atol"), "rtol": (t / fn, 0.0, "rtol"), "rtol wins": (t / fn, t / 4, "rtol"),
             "atol wins": (t / (4 * fn), t, "atol")}
    for name, (rtol, atol, reason) in cases.items():
        s, info, _ = _run(g_tri, kind, ipg, rtol=rtol, atol=atol)
        print(f"{name} ({kind}, ipg {ipg}): k {k}, threshold {t:.3e}, {info}")
        assert info.reason == reason and info.converged and info.iterations == k, (name, info, k)
        _assert_iterate(s, ref, k)
        st = s._read_status()
        assert st[R.ST_RTOLWINS] == (1.0 if reason == "rtol" else 0.0) and st[R.ST_RNORM] == info.residual_norm <= st[R.ST_TOL]
    # the tie: atol is the product the kernel forms from its own |f|, read back after a first _start; the second _start runs
    # on the same gradients (a solve() would form them again, and their last bits are not reproducible)
    s, _ = _make(kind, "reference", "block_jacobi", g_tri, tri_case=STOP_TRI_CASE, iters_per_graph=ipg)
    rtol = t / fn
    fn_dev = _prime(s, rtol, 0.0, 100)[R.ST_FNORM]
    atol = rtol * fn_dev
    st = _restart(s, rtol, atol, 100)
    assert st[R.ST_FNORM] == fn_dev and st[R.ST_TOL] == atol and st[R.ST_RTOLWINS] == 1.0
    st = _drive(s, 100)
    assert st[R.ST_REASON] == 1.0 and st[R.ST_HALTED] == 1.0 and st[R.ST_ITER] == float(k), (st, k)     # 1: "rtol"
    got = R.rel(s._u.cpu().numpy().reshape(-1), ref["hi"][k]["u"])
    assert got <= R.allowed(ref["dev"][k]["u"]), (k, got)
    _halted_for_good(s)


@pytest.mark.parametrize("ipg", [1, 16])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_max_iter_stops_at_exactly_that_iteration_also_inside_a_graph_and_at_zero(g_tri, kind, ipg):
    ref = _stop_reference(g_tri, kind)
    rtol = 1e-14
    assert min(float(r["rnorm"]) for r in ref["hi"][:6]) > 1e3 * rtol * float(ref["hi"][0]["fnorm"])    # not met by iteration 5
    s, info, _ = _run(g_tri, kind, ipg, rtol=rtol, max_iter=5)
    assert info.iterations == 5 and info.reason == "max_iter" and not info.converged, info
    _assert_iterate(s, ref, 5)
    st = s._read_status()
    assert st[R.ST_ITER] == 5.0 and st[R.ST_MAXITER] == 5.0 and _relerr(st[R.ST_RNORM], ref["hi"][5]["rnorm"]) <= \
        R.allowed(ref["dev"][5]["rnorm"])
    s, info, u0 = _run(g_tri, kind, ipg, rtol=rtol, max_iter=0)
    assert info.iterations == 0 and info.reason == "max_iter" and not info.converged, info
    assert torch.equal(s.model.u_free.detach(), u0)
    assert _relerr(info.residual_norm, ref["hi"][0]["rnorm"]) <= R.allowed(ref["dev"][0]["rnorm"])


@pytest.mark.parametrize("ipg", [1, 16])
@pytest.mark.parametrize("kind,precond", [("tri3", "block_jacobi"), ("quad4", "block_jacobi"), ("tri3_amg", "amg")])
def test_a_nan_in_the_start_is_a_breakdown_at_iteration_zero(g_tri, kind, precond, ipg):
    """One NaN in ``u_free``: dE/du and with it |r_0| are NaN, so the start halts with "breakdown" and nothing after it runs --
    with AMG neither a cycle launch nor the rho step.  ``u_free`` is as it was."""
    s, _ = _make(kind, "reference", precond, g_tri, iters_per_graph=ipg, rtol=1e-10)
    with torch.no_grad():
        s.model.u_free[3, 0] = float("nan")
    u0 = s.model.u_free.detach().clone()
    info = s.solve()
    assert info.reason == "breakdown" and info.iterations == 0 and not info.converged, info
    assert math.isnan(info.residual_norm) and math.isfinite(info.rhs_norm)
    assert torch.allclose(s.model.u_free.detach(), u0, rtol=0.0, atol=0.0, equal_nan=True)
    assert int(torch.isnan(s.model.u_free).sum()) == 1
    _halted_for_good_nan(s)


def _halted_for_good_nan(s):
    st0, u0 = s._read_status(), s._u.clone()
    assert st0[R.ST_HALTED] == 1.0
    for _ in range(3):
        s._replay()
    st1 = s._read_status()
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(st0, st1))
    assert torch.allclose(s._u, u0, rtol=0.0, atol=0.0, equal_nan=True)


@pytest.mark.parametrize("ipg", [1, 16])
def test_amg_start_inside_the_tolerance_does_no_iteration(g_tri, ipg):
    s, _ = _make("tri3_amg", "reference", "amg", g_tri, iters_per_graph=ipg, rtol=1e-10)
    assert s.solve().converged
    u1 = s.model.u_free.detach().clone()
    from hidenn_fem_amd.solve import FrozenMeshSolver
    warm = FrozenMeshSolver(s.model, s.loss_fn, precond="amg", rtol=1e-8, iters_per_graph=ipg)
    info = warm.solve()
    assert info.converged and info.reason == "rtol" and info.iterations == 0, info
    assert torch.equal(s.model.u_free.detach(), u1)
    _halted_for_good(warm)
