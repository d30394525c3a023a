"""The references, data, bounds and case builders of tests/adam_cases.py, checked on the CPU: what tests/test_gpu_adam_edges.py
holds the Adam kernels to is ``torch.optim.Adam``'s arithmetic, on entries that carry all their digits, at the sizes the
comments in csrc/optim.hip name."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import adam_cases as A

F32, F64 = torch.float32, torch.float64
ROOT = Path(__file__).resolve().parent.parent


def _torch_adam(groups, steps):
    """``groups``: list of (adam_data dict with zero state, hyper).  torch.optim.Adam(foreach=False) on the CPU, one parameter
    per group -> per group (p, exp_avg, exp_avg_sq) as numpy after ``steps`` steps."""
    params = [torch.from_numpy(d["p"].copy()).requires_grad_(True) for d, _ in groups]
    opt = torch.optim.Adam([dict(params=[p], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"]) for p, (_, h) in zip(params, groups)],
                           foreach=False)
    for k in range(steps):
        for p, (d, _) in zip(params, groups):
            p.grad = torch.from_numpy(d["grads"][k].copy())
        opt.step()
    return [(p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()) for p in params]


GROUPS = (A.HYPER, dict(A.HYPER, lr=3e-3), A.HYPER_B)        # two groups with different lr, and a betas=(0.0, 0.5) group


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_adam_numpy_is_torch_adam(dtype):
    """Five steps from a fresh state, three parameter groups: adam_numpy per entry within ADAM_RTOL of torch (fp64); in fp32
    torch within the allowance of adam_longdouble, and adam_numpy within the same of torch."""
    steps, n = 5, 20_000
    groups = [(A.adam_data(n, dtype, 300 + i, steps, zero_state=True), h) for i, h in enumerate(GROUPS)]
    got = _torch_adam(groups, steps)
    for i, ((d, h), res) in enumerate(zip(groups, got)):
        ref = A.run_steps(functools.partial(A.adam_numpy, dtype=A.NP[dtype]), d, steps, **h)[-1]
        ld = A.run_steps(A.adam_longdouble, d, steps, **h)[-1]
        allow = A.fp32_allowance(steps, True, h)
        for name, t, r, l in zip("pmv", res, ref, ld):
            e_ref, e_ld = A.rel_err(r, t), A.rel_err(t, l)
            print(f"group {i} {name} {dtype}: adam_numpy against torch {e_ref:.3e}, torch against longdouble {e_ld:.3e}")
            assert r.dtype == t.dtype == A.NP[dtype]
            if dtype == F64:
                assert e_ref <= A.ADAM_RTOL and e_ld <= A.ADAM_RTOL, (i, name)
            else:
                assert e_ref <= allow[name] and e_ld <= allow[name], (i, name, allow)
        assert np.abs(res[0] - d["p"]).max() <= 0.05 + 1e-6             # the stated total movement


def test_adam_numpy_generalises_adam_rows_numpy():
    d = A.adam_data(600, F64, 5)
    p, m, v = (d[k].reshape(300, 2) for k in "pmv")
    want = A.adam_rows_numpy(p, d["grads"][0].reshape(300, 2), m, v, np.arange(300), 3, **A.HYPER)
    got = A.adam_numpy(p, d["grads"][0].reshape(300, 2), m, v, 3, **A.HYPER)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_references_against_longdouble_and_the_fp32_allowance():
    """Records how far the restatements sit from longdouble on 200 000 non-cancelling entries over 5 steps (fp64: 7.5e-16;
    fp32: p 2.6e-7, m 1.5e-7, v 4.5e-7), and holds every fp32 allowance the GPU test uses between 1e-7 and 1e-5."""
    d = A.adam_data(A.ALLOW_N, F64, 1005, 5)
    ref, ld = A.run_steps(A.adam_numpy, d, 5, **A.HYPER)[-1], A.run_steps(A.adam_longdouble, d, 5, **A.HYPER)[-1]
    for name, r, l in zip("pmv", ref, ld):
        e = A.rel_err(r, l)
        print(f"fp64 adam_numpy against longdouble, 5 steps, {name}: {e:.3e}")
        assert e <= 2e-15                                            # a few roundings of 1.1e-16, far below ADAM_RTOL
    for steps, zero, h in [(5, False, A.HYPER), (A.STEPS, False, A.HYPER), (A.BIG_STEPS, False, A.HYPER), (6, True, A.HYPER),
                           (5, True, A.HYPER_B), (1, False, A.HYPER)] + [(A.STEPS, False, t[2]) for t in A.seven_tensors(256) if t[1] == F32] \
            + [(A.STEPS, False, dict(A.HYPER, lr=lr)) for lr in (A.LR_X, A.LR_U)]:
        allow = A.fp32_allowance(steps, zero, h)
        print(f"fp32 allowance ({A.FP32_FACTOR} x adam_numpy against longdouble), {steps} steps, zero state {zero}, "
              f"lr {h['lr']} betas ({h['beta1']}, {h['beta2']}): " + ", ".join(f"{k} {a:.3e}" for k, a in allow.items()))
        assert all(1e-7 <= a <= 1e-5 for a in allow.values()), allow


def test_fp32_statement_is_adam_one_float():
    """The fp32 form casts every scalar to float FIRST (float(1 - b1), not 1 - float(b1)) and takes the root in double."""
    w1, b2, w2, ss, sb, eps = A._scalars(3, 1e-2, 0.9, 0.999, 1e-8, np.float32)
    assert w1 == np.float32(1.0 - 0.9) and w2 == np.float32(1.0 - 0.999) and w2 != np.float32(1) - np.float32(0.999)
    assert ss == np.float32(1e-2 / (1 - 0.9 ** 3)) and sb == np.float32(np.sqrt(1 - 0.999 ** 3)) and eps == np.float32(1e-8)
    d = A.adam_data(1000, F32, 9)
    p, m, v = A.adam_numpy(d["p"], d["grads"][0], d["m"], d["v"], 1, **A.HYPER, dtype=np.float32)
    assert np.array_equal(v, d["v"] * b2 + w2 * (d["grads"][0] * d["grads"][0])) and v.dtype == np.float32


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_data_does_not_cancel(dtype):
    d = A.adam_data(5000, dtype, 17, 5)
    assert all(a.dtype == A.NP[dtype] and a.shape == (5000,) for a in [d["p"], d["m"], d["v"]] + d["grads"])
    assert (np.abs(d["p"]) >= 0.5).all() and (np.abs(d["p"]) < 1.5).all() and (d["v"] > 0).all()
    for g in d["grads"]:
        assert (np.sign(g) == np.sign(d["m"])).all() and (np.abs(g) >= 0.05).all()
    last = A.run_steps(A.adam_longdouble, d, 5, **A.HYPER)[-1]
    assert np.abs(last[0] - d["p"]).max() <= 0.05 and (np.sign(last[1]) == np.sign(d["m"])).all()
    again = A.adam_data(5000, dtype, 17, 5)
    assert all(np.array_equal(d[k], again[k]) for k in "pmv") and not np.array_equal(d["p"], A.adam_data(5000, dtype, 18, 5)["p"])
    z = A.adam_data(10, dtype, 17, zero_state=True)
    assert not z["m"].any() and not z["v"].any() and np.array_equal(z["p"], A.adam_data(10, dtype, 17)["p"])


def test_lengths_are_the_cap_and_one_trip_more():
    """The stated lengths: the grid cap exactly (one trip of the vector loop with all 2048 blocks), and cap + 256 vectors + a
    full tail (block 0 alone takes a second trip); an unaligned view of that length takes the scalar loop's second trip."""
    assert A.LENGTHS[F64][-2:] == (1_048_576, 1_049_089) and A.LENGTHS[F32][-2:] == (2_097_152, 2_098_179)
    for dt in (F64, F32):
        N, (cap, more) = A.VEC[dt], A.LENGTHS[dt][-2:]
        assert A.step_grid(cap, dt) == A.GRID_CAP == A.step_grid(more, dt) and A.step_grid(cap - N, dt) == A.GRID_CAP
        assert A.step_grid(cap - 256 * N, dt) == A.GRID_CAP - 1
        assert A.vector_trips(cap, dt) == 1 and A.vector_trips(cap + N, dt) == 2 and A.vector_trips(more, dt) == 2
        assert more // N - A.GRID_CAP * 256 == 256 and more % N == N - 1
        assert all(A.vector_trips(n, dt) <= 1 for n in A.LENGTHS[dt][:-2])
        assert {n % N for n in A.LENGTHS[dt]} == set(range(N))                         # every tail length
        assert A.steps_of(cap, dt) == A.BIG_STEPS and A.steps_of(A.OFFSET_N[dt], dt) == A.STEPS
    assert A.vector_trips(A.ONE_TRIP_MORE[F64], F64, aligned=False) >= 2


def test_row_lists_have_no_row_twice():
    for n_x, n_u in A.ROW_SPLITS:
        c = A.rows2_case(n_x, n_u, F64)
        rx, ru = c["rows_x"].long(), c["rows_u"].long()
        assert rx.shape[0] == n_x and ru.shape[0] == n_u and rx.dtype == torch.int64 and c["rows_x"].dtype == torch.int32
        assert torch.unique(rx).shape[0] == n_x and torch.unique(ru).shape[0] == n_u
        assert (n_x < 2 or not rx.equal(rx.sort().values)) and (n_u < 3 or not ru.equal(ru.sort().values))
        assert (n_x == 0 or (0 <= rx.min() and rx.max() < A.ROWS_X)) and (n_u == 0 or (0 <= ru.min() and ru.max() < A.ROWS_U))
    assert (100, 300) in A.ROW_SPLITS and 100 < 256 < 400                  # the x/u split inside block 0
    assert A.LR_X != A.LR_U


@pytest.mark.parametrize("chunk", A.CHUNKS)
def test_block_tables_cover_every_vector_exactly_once(chunk):
    tensors = A.seven_tensors(chunk)
    begin, need = A.table_layout(tensors, chunk)
    assert len(tensors) == 7 and begin[0] == 0 and all(b > a for a, b in zip(begin, begin[1:]))       # every tensor >= 1 block
    assert sum(t[0] for t in tensors) < 100_000
    for n_blocks in (need, need + 5):                            # idle blocks land behind the last tensor's chunk: no work
        for (n, *_), count in zip(tensors, A.table_cover(tensors, chunk, n_blocks)):
            assert count.shape == (n,) and (count == 1).all()
    short = A.table_cover(tensors, chunk, need - 1)
    assert (short[-1] == 0).any()                                # the count is the table's NEED: one block fewer misses a vector
    if chunk == 512:
        assert A.blocks_needed(3001, F64, 512) == 3 and 1500 - 2 * 512 == 476          # second and third trips, a partial last block
    assert tensors[4][3] == 1 and tensors[4][4] == 2 and A.blocks_needed(700, F64, chunk, aligned=False) == 1
    assert tensors[6][0] // 2 == chunk and A.blocks_needed(tensors[6][0], F64, chunk) == 1


def test_fused_table_layout_at_chunk_512():
    chunk, begin, blocks = A.fused_table_layout([1_048_578, 37], [F64, F32])
    assert chunk == 512 and begin == [0, 1025] and blocks == 1026


def test_special_values_through_the_references():
    """What "expected" means in E: adam_numpy's value, entry by entry."""
    for dtype in (F64, F32):
        T = A.NP[dtype]
        res = {}
        for name, c in A.special_cases(dtype):
            res[name] = A.adam_numpy(c["p"], c["g"], c["m"], c["v"], c["step"], **c["hyper"], dtype=T)
            assert all(a.dtype == T for a in res[name])
        c = dict(A.special_cases(dtype))
        z = c["zero gradient, zero state"]
        for got, init in zip(res["zero gradient, zero state"], (z["p"], z["m"], z["v"])):
            assert got.tobytes() == init.tobytes()
        p, m, v = res["g*g overflows"]
        assert np.isposinf(v).all() and np.array_equal(p, c["g*g overflows"]["p"]) and np.isfinite(m).all() and (m != 0).all()
        s = c["step 10^6"]
        w1, b2, w2, step_size, sqrt_bc2, eps = A._scalars(s["step"], **s["hyper"], T=T)
        assert sqrt_bc2 == 1 and step_size == T(s["hyper"]["lr"])
        p, m, v = res["beta1 = 0"]
        assert A.rel_err(m, c["beta1 = 0"]["g"]) <= (1e-15 if dtype == F64 else 1e-6)
        p, m, v = res["eps = 0"]
        assert np.isfinite(p).all() and (p != c["eps = 0"]["p"]).all()
        if dtype == F32:
            p, m, v = res["g*g underflows"]
            assert not v.any() and (np.abs(m) >= np.finfo(np.float32).tiny).all() and np.array_equal(p, c["g*g underflows"]["p"])


def test_ticket_constant_is_the_header_one():
    from hidenn_fem_amd import _lib
    text = (ROOT / "include" / "hidenn_fem.h").read_text()
    assert int(re.search(r"#define\s+HFEM_ADAM_TICKET_INTS\s+(\d+)", text).group(1)) == _lib.ADAM_TICKET_INTS
    assert _lib.ADAM_TICKET_INTS >= 32 * (1 + A.TICKET_CLASSES)           # one 128-byte line per class and one for the top counter
    assert "1056" not in (ROOT / "hidenn_fem_amd" / "optim.py").read_text()
