"""tests/lbfgs_reference.py pinned without a GPU: run free (its own direction fed back) it follows ``torch.optim.LBFGS`` on
the CPU -- losses, parameters, n_iter and the number of pairs kept, to the tolerances tests/test_gpu_lbfgs.py holds
FusedLBFGS to against torch --, it states the rejected-pair rule and the g.d stop, and three mutations of it (``>=`` in the
acceptance rule, the newest pair left out of the first loop, H_diag not refreshed) each break the comparison with torch, so
the comparison is able to see them.  Full histories (last section): the stiff chain fills every history
tests/test_gpu_lbfgs_histories.py runs, the reference follows torch iteration by iteration at 100 and 257 full pairs, and the
coefficient-space form the kernels evaluate fits half of that file's tolerance when stated in plain float64."""
import numpy as np
import pytest
import torch

import lbfgs_reference as R
from test_gpu_lbfgs import _quadratic

CPU = torch.device("cpu")


def _drive(ref, fun, x0, n_steps, max_iter=20):
    """``n_steps`` x ``torch.optim.LBFGS.step(closure)`` as torch/optim/lbfgs.py sequences it, on the reference's check /
    direction / apply_update.  Returns the steps' first losses and the final parameters."""
    x, losses, max_eval = x0.copy(), [], max_iter * 5 // 4          # torch's default
    for _ in range(n_steps):
        loss, g = fun(x)
        losses.append(loss)
        evals = 1
        if int(ref.check(g, loss, after_update=False)[R.ST_FLAGS]) & R.F_OPT:
            continue
        n_iter = 0
        while n_iter < max_iter:
            n_iter += 1
            out = ref.direction(g)
            if out["stop_gtd"]:
                break
            x = R.apply_update(x, out["d"], out["t"])
            if n_iter == max_iter:
                break
            loss, g = fun(x)
            evals += 1
            flags = int(ref.check(g, loss)[R.ST_FLAGS])
            if evals >= max_eval or flags & (R.F_OPT | R.F_STEP | R.F_LOSS):
                break
    return losses, x


def _torch_run(fun, x0, n_steps, **kw):
    p = torch.nn.Parameter(torch.from_numpy(x0.copy()))
    opt = torch.optim.LBFGS([p], **kw)
    losses = []

    def closure():
        loss, g = fun(p.detach().numpy())
        p.grad = torch.from_numpy(g.copy())
        return torch.tensor(loss, dtype=torch.float64)

    for _ in range(n_steps):
        losses.append(opt.step(closure).item())
    st = opt.state[p]
    return losses, p.detach().numpy().copy(), st["n_iter"], len(st.get("old_dirs") or [])


def _quadratic_fun():
    """``_quadratic`` of tests/test_gpu_lbfgs.py (n = 87, two parameter tensors) as a function of the flat vector."""
    params, f = _quadratic(CPU, torch.float64)
    x0 = torch.cat([p.detach().reshape(-1) for p in params]).numpy().copy()

    def fun(x):
        t = torch.from_numpy(x.copy()).requires_grad_(True)
        loss = f(t[:37], t[37:].reshape(25, 2))
        g, = torch.autograd.grad(loss, t)
        return loss.item(), g.numpy().copy()

    return fun, x0


def _chain_fun(n=4097):
    prob = R.ChainProblem(n)
    return prob.loss_and_grad, prob.x0.copy()


def _compare(ref_cls, fun, x0, history, n_steps, dtype=np.float64):
    """The torch comparison: AssertionError unless the reference follows torch.optim.LBFGS."""
    ref = ref_cls(history, dtype=dtype)
    got_l, got_x = _drive(ref, fun, x0, n_steps)
    want_l, want_x, want_iter, want_pairs = _torch_run(fun, x0, n_steps, history_size=history)
    assert got_l[0] == want_l[0]
    np.testing.assert_allclose(got_l, want_l, rtol=1e-9, atol=1e-9)               # test_gpu_lbfgs.py: fused against torch
    np.testing.assert_allclose(got_x.astype(np.float64), want_x, rtol=1e-7, atol=1e-9)
    assert (ref.n_iter, ref.count) == (want_iter, want_pairs)
    assert want_l[-1] < want_l[0] - 1.0                                           # the optimiser really moved
    return ref


CASES = {"quadratic87": (_quadratic_fun, 4), "chain4097": (_chain_fun, 2)}


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["float64", "longdouble"])
@pytest.mark.parametrize("history", [3, 100])
@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_follows_torch_lbfgs(case, history, dtype):
    make, n_steps = CASES[case]
    fun, x0 = make()
    ref = _compare(R.LbfgsReference, fun, x0, history, n_steps, dtype=dtype)
    assert 0 < ref.count <= min(history, ref.n_iter - 1)


def test_chain_problem_is_what_the_gpu_test_needs():
    """The properties tests/test_gpu_lbfgs_lengths.py relies on, at a length with the same statistics: the gradient is the
    derivative of the loss, every pair is accepted, no break flag fires in history + 3 iterations, the first step takes the
    1 / |g|_1 branch and g.d < 0 throughout."""
    R.assert_longdouble_is_wider()
    prob = R.ChainProblem(4097)
    x = prob.x0.copy()
    _, g = prob.loss_and_grad(x)
    v = np.random.default_rng(1).standard_normal(x.size)
    h = 1e-6
    fd = (prob.loss_and_grad(x + h * v)[0] - prob.loss_and_grad(x - h * v)[0]) / (2 * h)
    assert abs(fd - g @ v) <= 1e-6 * abs(g @ v)
    for T in (np.float64, np.float32):
        ref, x = R.LbfgsReference(5), prob.x0.astype(T)
        for k in range(8):
            loss, g = prob.loss_and_grad(x)
            assert g.dtype == T and float(T(loss)) == loss
            out = ref.iterate(g, loss)
            assert out["status"][R.ST_FLAGS] == 0 and out["gtd"] < 0 and not out["stop_gtd"]
            assert out["accepted"] is (None if k == 0 else True)
            assert (out["t"] < 1e-3) if k == 0 else (out["t"] == 1.0)
            x = R.apply_update(x, out["d"], out["t"])
        assert ref.count == 5 and ref.n_iter == 8


def test_rejected_pair_and_gtd_stop_are_stated():
    """The same gradient twice: y = 0, the pair is dropped, history and H_diag stay, the direction is the one before; a
    tolerance_change above -g.d sets the stop, and the next check reports bit 3.  The sharded entry takes the break tests
    first: when one fires nothing moves and bit 4 is set."""
    prob = R.ChainProblem(257)
    for entry in ("iterate", "shard_iterate"):
        ref, x = R.LbfgsReference(3), prob.x0.copy()
        for k in range(5):
            loss, g = prob.loss_and_grad(x)
            out = getattr(ref, entry)(g, loss, **({} if entry == "iterate" else dict(after_update=k > 0)))
            x = R.apply_update(x, out["d"], out["t"])
        loss, g = prob.loss_and_grad(x)
        out = getattr(ref, entry)(g, loss - 1.0)
        S, Y, H, d, n_iter = list(ref.S), list(ref.Y), ref.H_diag, out["d"].copy(), ref.n_iter
        assert out["accepted"] is True and ref.count == 3
        again = getattr(ref, entry)(g, loss - 2.0)                                # no apply in between
        assert again["accepted"] is False and ref.n_iter == n_iter + 1
        assert all(a is b for a, b in zip(ref.S + ref.Y, S + Y)) and ref.count == 3 and ref.H_diag == H
        assert np.array_equal(again["d"], d) and again["t"] == 1.0 and again["gtd"] == out["gtd"]
        kw = {} if entry == "iterate" else dict(after_update=False)               # (sharded: 1e30 would fire the break tests)
        stop = getattr(ref, entry)(g, loss - 3.0, tolerance_change=1e30, **kw)
        assert stop["stop_gtd"] and stop["gtd"] < 0 and not out["stop_gtd"]
        if entry == "iterate":
            assert int(ref.check(g, loss - 4.0)[R.ST_FLAGS]) == R.F_GTD
        else:
            assert int(stop["status"][R.ST_FLAGS]) == R.F_GTD
            before = (ref.n_iter, ref.count, ref.H_diag, ref.prev_g, ref.prev_loss)
            for kw in (dict(want_direction=False), dict()):                       # the host's wish; the loss-change test (same loss)
                skip = ref.shard_iterate(g, ref.prev_loss + (1.0 if kw else 0.0), **kw)
                assert skip["d"] is None and int(skip["status"][R.ST_FLAGS]) == R.F_NODIR + (0 if kw else R.F_LOSS)
                assert before[:3] == (ref.n_iter, ref.count, ref.H_diag) and ref.prev_g is before[3] and ref.prev_loss == before[4]


def test_apply_update_fused_form_is_one_rounding():
    rng = np.random.default_rng(3)
    x, d = rng.standard_normal(4000), rng.standard_normal(4000)
    t = 0.37
    fused, plain = R.apply_update(x, d, t, fused=True), R.apply_update(x, d, t)
    exact = np.array([R.apply_update_exact(a, b, t) for a, b in zip(x, d)])
    assert np.array_equal(fused, exact)
    assert 0 < (plain != exact).sum() < 2000 and np.abs(plain - exact).max() <= np.spacing(np.abs(exact)).max()
    assert np.array_equal(R.apply_update(x, d, 1.0, fused=True), x + d)           # t = 1: the product is exact
    x32, d32 = x.astype(np.float32), d.astype(np.float32)
    assert R.apply_update(x32, d32, t, fused=True).dtype == np.float32


# ------------------------------------------------------------------------------------------------ mutation checks
class _AcceptEqual(R.LbfgsReference):
    def _accept(self, ys):
        return ys >= 1e-10


class _NewestPairLeftOut(R.LbfgsReference):
    def _first_loop(self, m):
        return range(m - 2, -1, -1)


class _StaleH(R.LbfgsReference):
    def _refreshed_h(self, ys, yy):
        return self.H_diag


def _scripted():
    """Gradients that do not depend on x, built so that the second iteration's y.s is EXACTLY 1e-10: g0 = (-0.5, -1e-10) gives
    t = 1 (|g0|_1 < 1), s = (0.5, 1e-10); g1 = (-0.5, fl(1 - 1e-10)) gives y = (0, 1)."""
    gs = [np.array([-0.5, -1e-10]), np.array([-0.5, 1.0 - 1e-10]), np.array([0.25, -0.3]), np.array([0.1, 0.1])]
    calls = []

    def fun(x):
        calls.append(1)
        k = min(len(calls), len(gs)) - 1
        return 10.0 - 2.0 * k, gs[k].copy()

    y, s = gs[1] - gs[0], -gs[0] * 1.0
    assert np.array_equal(y, [0.0, 1.0]) and (y * s).sum() == 1e-10
    return fun, np.zeros(2), calls


def _compare_scripted(ref_cls):
    fun, x0, calls = _scripted()
    ref = ref_cls(5)
    _, got_x = _drive(ref, fun, x0, 1, max_iter=4)
    del calls[:]
    _, want_x, want_iter, want_pairs = _torch_run(fun, x0, 1, history_size=5, max_iter=4)
    np.testing.assert_allclose(got_x, want_x, rtol=1e-7, atol=1e-9)
    assert (ref.n_iter, ref.count) == (want_iter, want_pairs) == (4, 2)           # torch dropped the y.s = 1e-10 pair, kept the next


def test_acceptance_rule_is_strict_on_a_constructed_ys():
    _compare_scripted(R.LbfgsReference)


def test_mutation_accept_equal_breaks_the_torch_comparison():
    with pytest.raises(AssertionError):
        _compare_scripted(_AcceptEqual)


@pytest.mark.parametrize("mutant", [_NewestPairLeftOut, _StaleH])
@pytest.mark.parametrize("case", sorted(CASES))
def test_mutation_breaks_the_torch_comparison(case, mutant):
    make, n_steps = CASES[case]
    fun, x0 = make()
    _compare(R.LbfgsReference, fun, x0, 3, n_steps)                               # the comparison itself holds ...
    with pytest.raises(AssertionError):                                           # ... and sees the mutation
        _compare(mutant, fun, x0, 3, n_steps)


# ------------------------------------------------------------------------------------------------ full histories (stiff chain)
def _history_cases():
    """Every (n, T, history, iterations) tests/test_gpu_lbfgs_histories.py runs (the same lists: the two cannot drift)."""
    f = R.HISTORY_FUSED
    cases = list(R.HISTORY_UNSHARDED) + [(sum(lengths), T, h, it) for lengths, T, h, it in R.HISTORY_SHARDED]
    return cases + [(f["n"], np.float64, f["history"], f["max_iter"])]


def _case_id(case):
    n, T, history, iters = case
    return f"n{n}-{T.__name__}-h{history}-it{iters}"


@pytest.mark.parametrize("n", sorted({c[0] for c in _history_cases()}))
def test_stiff_chain_gradient_is_the_derivative_of_its_loss(n):
    prob = R.stiff_chain(n)
    assert prob.a.min() >= 1.0 and prob.a.max() > 5e4 and np.array_equal(prob.b, R.ChainProblem(n, seed=R.STIFF_SEED).b)
    x = prob.x0.copy()
    _, g = prob.loss_and_grad(x)
    v = np.random.default_rng(1).standard_normal(n)
    h = 1e-6
    fd = (prob.loss_and_grad(x + h * v)[0] - prob.loss_and_grad(x - h * v)[0]) / (2 * h)       # exact for a quadratic, but for rounding
    assert abs(fd - g @ v) <= 1e-6 * abs(g @ v)


@pytest.mark.parametrize("case", _history_cases(), ids=_case_id)
def test_stiff_chain_fills_the_history_the_gpu_test_needs(case):
    """Free float64 run on the stiff chain: every pair is accepted, no break flag fires, g.d stays below -1e-3 (far from
    -tolerance_change), the history is full from iteration ``history`` on, the first step takes the 1 / |g|_1 branch."""
    n, T, history, iters = case
    assert iters >= history + 3
    prob = R.stiff_chain(n)
    ref, x = R.LbfgsReference(history), prob.x0.astype(T)
    for k in range(iters):
        loss, g = prob.loss_and_grad(x)
        assert g.dtype == T and float(T(loss)) == loss
        out = ref.iterate(g, loss)
        assert out["status"][R.ST_FLAGS] == 0 and not out["stop_gtd"], (k, out["status"])
        assert out["gtd"] < -1e-3, (k, out["gtd"])
        assert out["accepted"] is (None if k == 0 else True), k
        assert out["count"] == min(k, history), (k, out["count"])
        assert (out["t"] < 1e-3) if k == 0 else (out["t"] == 1.0)
        x = R.apply_update(x, out["d"], out["t"])
    assert ref.count == history and ref.n_iter == iters


def _pin_against_torch_per_iteration(ref_cls, history, iters, n=1031):
    """``torch.optim.LBFGS(max_iter=1)`` one ``step`` at a time (its state persists: the same recursion as one long step, the
    direction and the step readable after every iteration).  Free trajectories of torch and the reference drift apart by
    rounding amplified over hundreds of iterations (1e-3 of max|x| after 260 on this problem), so the float64 and the
    longdouble reference are FED torch's d and t -- their history then has torch's bits -- and torch's d, scaled by the summed
    magnitudes of its terms, must be within ``R.allowed`` of the gap between the two; accepted flags and pair counts equal."""
    R.assert_longdouble_is_wider()
    prob = R.stiff_chain(n)
    p = torch.nn.Parameter(torch.from_numpy(prob.x0.copy()))
    opt = torch.optim.LBFGS([p], max_iter=1, history_size=history)
    seen = {}

    def closure():
        seen["loss"], seen["g"] = prob.loss_and_grad(p.detach().numpy().copy())
        p.grad = torch.from_numpy(seen["g"].copy())
        return torch.tensor(seen["loss"], dtype=torch.float64)

    r64, rld = ref_cls(history, np.float64), ref_cls(history, np.longdouble)
    d_prev = t_prev = None
    worst = [0.0, 0.0]
    for k in range(iters):
        opt.step(closure)
        st = opt.state[p]
        d_torch, t_torch = st["d"].numpy().copy(), float(st["t"])
        assert st["n_iter"] == k + 1
        o64, old = (r.iterate(seen["g"], seen["loss"], d_prev, t_prev) for r in (r64, rld))
        assert o64["accepted"] is old["accepted"] is (None if k == 0 else True), k
        assert o64["count"] == old["count"] == len(st.get("old_dirs") or []) == min(k, history), k
        t_ld = float(old["t"])                                                    # (1 / |g|_1 at k = 0: the sum's rounding; then lr)
        assert abs(t_torch - t_ld) <= R.allowed(abs(float(o64["t"]) - t_ld) / t_ld) * t_ld and (k == 0 or t_torch == 1.0), k
        scale = np.maximum(r64.term_magnitudes(seen["g"]), np.finfo(np.float64).tiny)
        gap = float((np.abs(r64.r.astype(np.longdouble) - rld.r) / scale).max())
        err = float((np.abs(d_torch.astype(np.longdouble) - rld.r) / scale).max())
        worst = [max(worst[0], err), max(worst[1], gap)]
        assert err <= R.allowed(gap), (k, err, gap, R.allowed(gap))
        d_prev, t_prev = d_torch, t_torch
    assert r64.count == history and len(opt.state[p]["old_dirs"]) == history
    print(f"LBFGS-TORCH-PIN h{history}: torch {worst[0]:.2e} reference {worst[1]:.2e}")


@pytest.mark.parametrize("history", [100, 257])
def test_reference_follows_torch_iteration_by_iteration_at_a_full_history(history):
    _pin_against_torch_per_iteration(R.LbfgsReference, history, history + 3)


@pytest.mark.parametrize("mutant", [_NewestPairLeftOut, _StaleH])
def test_mutation_breaks_the_per_iteration_torch_pin(mutant):
    """(``_AcceptEqual`` cannot show here: no y.s of this problem is exactly 1e-10; the scripted case above holds it.)"""
    with pytest.raises(AssertionError):
        _pin_against_torch_per_iteration(mutant, 100, 103)


COEFFICIENT_CASES = [(1031, np.float64, 65), (1031, np.float64, 128), (1031, np.float64, 257), (1031, np.float32, 100),
                     (1031, np.float32, 129), (1031, np.float32, 257), (4096, np.float32, 128)]


@pytest.mark.parametrize("case", COEFFICIENT_CASES, ids=lambda c: f"n{c[0]}-{c[1].__name__}-h{c[2]}")
def test_coefficient_space_form_fits_half_the_tolerance(case):
    """The kernels run the recursion on Gram entries, not on vectors.  A plain float64 numpy statement of THAT form
    (``R.coefficient_direction``), on the history the float64 reference accumulates in a free run on the stiff chain, stays
    within 0.5 x ``R.allowed`` of the longdouble vector-space run, d and g.d, every 7th iteration and the last four: the form
    itself does not use up the tolerance tests/test_gpu_lbfgs_histories.py keeps (MARGIN = 32), so a kernel that exceeds it
    is wrong.  Worst share of ``allowed`` per case is printed."""
    n, T, history = case
    R.assert_longdouble_is_wider()
    prob = R.stiff_chain(n)
    r64, rld = R.LbfgsReference(history, np.float64), R.LbfgsReference(history, np.longdouble)
    x, iters = prob.x0.astype(T), history + 3
    d_prev = t_prev = None
    share = {"d": 0.0, "gtd": 0.0}
    for k in range(iters):
        loss, g = prob.loss_and_grad(x)
        o64 = r64.iterate(g, loss)
        old = rld.iterate(g, loss, d_prev, t_prev)                                 # the float64 run's history, longdouble arithmetic
        assert o64["accepted"] is old["accepted"] and o64["count"] == old["count"] == min(k, history)
        if k % 7 == 0 or k >= iters - 4:
            d, gtd, H = R.coefficient_direction(r64.S, r64.Y, g)
            scale = np.maximum(r64.term_magnitudes(g), np.finfo(np.float64).tiny)
            gtd_scale = float((np.abs(g.astype(np.float64)) * scale).sum())
            ld = np.longdouble
            for what, got, a, b, sc in (("d", d, r64.r, rld.r, scale), ("gtd", gtd, r64.gtd, rld.gtd, gtd_scale)):
                gap = float((np.abs(np.asarray(a, dtype=ld) - b) / sc).max())
                err = float((np.abs(np.asarray(got, dtype=ld) - b) / sc).max())
                share[what] = max(share[what], err / R.allowed(gap))
                assert err <= 0.5 * R.allowed(gap), (k, what, err, gap)
            assert abs(H - float(rld.H_diag)) <= 0.5 * R.allowed(abs(float(r64.H_diag) - float(rld.H_diag)) / float(rld.H_diag)) * float(rld.H_diag)
        d_prev, t_prev = o64["d"], o64["t"]
        x = R.apply_update(x, o64["d"], o64["t"])
    print(f"LBFGS-COEFFICIENT n{n} {T.__name__} h{history}: share of allowed  d {share['d']:.2f}  g.d {share['gtd']:.2f}")
