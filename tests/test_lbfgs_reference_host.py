"""tests/lbfgs_reference.py pinned without a GPU: run free (its own direction fed back) it follows ``torch.optim.LBFGS`` on
the CPU -- losses, parameters, n_iter and the number of pairs kept, to the tolerances tests/test_gpu_lbfgs.py holds
FusedLBFGS to against torch --, it states the rejected-pair rule and the g.d stop, and three mutations of it (``>=`` in the
acceptance rule, the newest pair left out of the first loop, H_diag not refreshed) each break the comparison with torch, so
the comparison is able to see them."""
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
