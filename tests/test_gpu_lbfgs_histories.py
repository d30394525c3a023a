"""The L-BFGS recursion kernels (csrc/lbfgs.hip) with their history FULL, step by step through the C ABI against
tests/lbfgs_reference.py.  ``launch_recursion`` picks one of four kernels by ``history_size``:
  wave1      recursion_wave_kernel<1>   history <= 64          one row per lane
  wave2      recursion_wave_kernel<2>   65 ... 128             two rows per lane, rows >= 64 published from the second register
  rank1      recursion_rank1_kernel     129 ... 256            256 threads, one row each
  reduction  recursion_kernel           > 256                  strided loops on one wave
and each differs from the others only once the number of live pairs reaches its range.  The rest of the suite selects them
(tests/test_gpu_lbfgs.py) but never holds more than 60 pairs, and tests/test_gpu_lbfgs_lengths.py, the only file that
compares with a reference, uses histories 5 and 8: its ChainProblem converges before 20 pairs are kept.  The STIFF chain
(``R.stiff_chain``: a ~ 10 ** U(0, 5)) keeps accepting pairs for hundreds of iterations; tests/test_lbfgs_reference_host.py
asserts that for every case below (the case lists live in tests/lbfgs_reference.py, one place for both files), pins the
reference against torch iteration by iteration at 257 full pairs, and shows that a plain float64 statement of the
coefficient-space form stays within half the tolerance used here.

Harness, comparisons and tolerances are those of tests/test_gpu_lbfgs_lengths.py, imported, not copied: status slots, flags,
count, n_iter and the applied parameters bit for bit; d, g.d, t, H_diag to ``R.allowed(dev, MARGIN = 32)`` (+ one fp32 ulp
for an fp32 d); both reference runs fed the device's own d and t.

Unsharded, n = 1031 (prime: a ragged tail in every pass; 16 slot classes in the multidot pass, so 257 pairs give nine trips
of its two-slot pipeline), histories 64, 65, 100, 128, 129, 256, 257 in fp64 and fp32: history + 3 applied iterations (every
count from 0 to history, the ring drops its oldest pair three times), a direction without apply, the same gradient again
(rejected at a full ring: d, count, H_diag stay), the g.d stop.  Histories 65, 100, 129 run 2 (history + 1) + 3 iterations:
head passes through every slot, wraps from M1 - 1 to 0 with a full ring, ``slot_of``'s x >= M1 branch is taken for every row.
Sharded flow, n = 1030: world 1 at histories 100 and 257, two handles (686 + 344) at 129; payload 5 M1 + 8 doubles.
``FusedLBFGS`` through its Python driver: ONE step of 106 iterations at history 100 on the same chain as a torch closure
over two parameter tensors (37 + 994); the recorded (g, loss) sequence replayed through a fresh handle over the C ABI must
give the recorded parameters bit for bit at every evaluation (every reduction in csrc/lbfgs.hip has a fixed order).

MEASURED on an MI355X (worst over a case's iterations of: the kernels' deviation / the float64 reference's own deviation, both
from the longdouble run, in the scales of the lengths file; the file takes 15 s, its slowest case 1.9 s):
  unsharded, n = 1031              d                  g.d                t                  H_diag
  wave1     h64  fp64  it 67      1.9e-15 / 2.3e-15  2.3e-16 / 1.2e-16  1.3e-16 / 1.3e-16  3.7e-16 / 2.7e-16
  wave1     h64  fp32  it 67      5.8e-08 / 2.0e-15  1.2e-16 / 1.7e-16  5.0e-17 / 5.0e-17  3.5e-16 / 2.6e-16
  wave2     h65  fp64  it 135     2.5e-15 / 3.0e-15  2.3e-16 / 1.2e-16  1.3e-16 / 1.3e-16  4.2e-16 / 2.8e-16
  wave2     h65  fp32  it 135     5.8e-08 / 4.6e-15  1.2e-16 / 1.7e-16  5.0e-17 / 5.0e-17  4.8e-16 / 3.1e-16
  wave2     h100 fp64  it 205     1.9e-15 / 9.0e-15  2.3e-16 / 1.2e-16  1.3e-16 / 1.3e-16  3.7e-16 / 4.7e-16
  wave2     h100 fp32  it 205     5.8e-08 / 5.5e-15  1.2e-16 / 1.7e-16  5.0e-17 / 5.0e-17  3.8e-16 / 4.1e-16
  wave2     h128 fp64  it 131     2.2e-15 / 4.1e-15  2.3e-16 / 1.2e-16  1.3e-16 / 1.3e-16  3.7e-16 / 4.7e-16
  wave2     h128 fp32  it 131     5.8e-08 / 4.1e-15  1.2e-16 / 1.7e-16  5.0e-17 / 5.0e-17  3.8e-16 / 4.1e-16
  rank1     h129 fp64  it 263     2.6e-15 / 1.2e-14  2.3e-16 / 1.2e-16  1.3e-16 / 1.3e-16  4.1e-16 / 5.0e-16
  rank1     h129 fp32  it 263     5.8e-08 / 5.7e-15  1.2e-16 / 1.7e-16  5.0e-17 / 5.0e-17  4.2e-16 / 5.2e-16
  rank1     h256 fp64  it 259     9.6e-15 / 2.8e-14  2.3e-16 / 1.2e-16  1.3e-16 / 1.3e-16  4.1e-16 / 4.7e-16
  rank1     h256 fp32  it 259     5.8e-08 / 1.6e-14  1.2e-16 / 1.7e-16  5.0e-17 / 5.0e-17  4.0e-16 / 4.1e-16
  reduction h257 fp64  it 260     9.5e-15 / 2.4e-14  1.6e-16 / 1.5e-16  1.3e-16 / 1.3e-16  4.1e-16 / 5.3e-16
  reduction h257 fp32  it 260     5.8e-08 / 1.6e-14  1.9e-16 / 1.7e-16  5.0e-17 / 5.0e-17  4.0e-16 / 4.1e-16
  sharded, world 1, n = 1030       d                  g.d                t                  H_diag
  wave2     h100 fp64  it 103     2.6e-15 / 2.4e-15  2.4e-16 / 1.8e-16  9.0e-17 / 9.0e-17  2.9e-16 / 4.7e-16
  wave2     h100 fp32  it 103     5.8e-08 / 2.4e-15  1.6e-16 / 1.6e-16  2.9e-17 / 2.9e-17  3.1e-16 / 3.2e-16
  reduction h257 fp64  it 260     5.6e-15 / 1.7e-14  1.8e-16 / 1.6e-16  9.0e-17 / 9.0e-17  4.1e-16 / 4.7e-16
  reduction h257 fp32  it 260     5.8e-08 / 2.0e-14  1.7e-16 / 1.6e-16  2.9e-17 / 2.9e-17  3.7e-16 / 3.2e-16
  sharded, world 2, n = 686+344    d                  g.d                t                  H_diag
  rank1     h129 fp64  it 132     3.0e-15 / 4.4e-15  2.1e-16 / 1.5e-16  9.4e-17 / 9.0e-17  3.3e-16 / 7.1e-16
  rank1     h129 fp32  it 132     5.8e-08 / 5.3e-15  1.5e-16 / 1.6e-16  2.9e-17 / 2.9e-17  3.9e-16 / 3.2e-16
The kernels stay at or below the float64 reference's own gap in d (which grows with the history: 2e-15 at 64 pairs, 2-3e-14
at 256); MARGIN = 32 is not needed by them and stays.  A case allows 3e-14 ... 9e-13 (fp32 d: 1.2e-7).  The replay test passed
bit for bit at all 106 evaluations.  No defect was found in csrc/lbfgs.hip.

MUTANTS of a scratch copy of csrc/lbfgs.hip, each run against the existing GPU L-BFGS tests (test_gpu_lbfgs.py without its
multi-process test, whose workers load the product library; test_gpu_lbfgs_lengths.py; the L-BFGS cases of
test_gpu_edge_cases.py: 37 tests) and against this file:
  1  recursion_wave_kernel<2> always publishes al_i from row register 0 (the else of its first loop deleted): all 37 existing
     tests pass; here the 8 wave2 cases fail (histories 65, 100, 128 unsharded, 100 sharded; fp64 and fp32), at k = 65, the
     first iteration with 65 live pairs: d off by 0.27 ... 0.69 of its scale where 3.4e-14 (fp32 d: 1.2e-7) is allowed.
  2  recursion_rank1_kernel skips the Gram write SY[j][new] for rows k >= 64: all 37 existing tests pass; here the 6 rank1 cases
     fail (129 and 256 unsharded, 129 with two handles), at k = 66: d off by 0.20 ... 0.50 where 7.0e-14 is allowed.
  3  multidot_kernel reduces the third and later slots of a class through ``red`` buffer 0 whatever their parity: this only
     removes the double buffering -- a race between the five threads that still read buffer 0 and the waves that write the next
     slot's sums -- and it did not show: all existing tests and all 21 cases here pass.  NO test sees this mutant.
  4  (own, same pipeline, deterministic) the prefetch of the slot after next is left out from a class's fifth slot on, so
     that slot is reduced from stale registers: the existing lengths file already sees it where gy = 1 gives a class five
     slots (4 of its cases fail, n = 2 097 154: d off by 0.19 where 3.7e-14 is allowed); here every case with more than 64
     pairs fails at k = 65 (19 of 21, the replay test included: the trajectory stops early; d off by 0.22 ... 0.61), the two
     wave1 cases (at most four slots per class) pass.
  5  (own, same pipeline) the same omission from a class's NINTH slot on, a depth no existing test reaches (at most six slots
     per class, in the sharded gy = 1 cases of the lengths file): all 37 existing tests pass; here the 10 cases with more than
     128 pairs fail (rank1 129 and 256, reduction 257, unsharded and sharded), at k = 129, the first iteration in which class 0
     holds nine slots: d off by 0.49 ... 0.97 where 8.0e-14 (fp32 d: 1.2e-7) is allowed."""
import numpy as np
import pytest
import torch

import lbfgs_reference as R
import test_gpu_lbfgs_lengths as LEN

F64, F32 = np.float64, np.float32
K_REC_WAVE_MAX, K_REC_MAX = 128, 256                       # kRecWaveMax, kRecMax


def _recursion_form(history):
    """``launch_recursion``'s choice (csrc/lbfgs.hip), restated."""
    if history > K_REC_MAX:
        return "reduction"
    if history > K_REC_WAVE_MAX:
        return "rank1"
    return "wave1" if history <= 64 else "wave2"


KERNEL = {64: "wave1", 65: "wave2", 100: "wave2", 128: "wave2", 129: "rank1", 256: "rank1", 257: "reduction"}


def _tname(T):
    return "fp64" if T == F64 else "fp32"


def _id(case):
    n, T, history, iters = case
    n = "+".join(str(v) for v in n) if isinstance(n, tuple) else n
    return f"{KERNEL[history]}-h{history}-{_tname(T)}-n{n}-it{iters}"


def _assert_case(lengths, T, history, iters):
    assert _recursion_form(history) == KERNEL[history]
    assert iters >= history + 3
    for n in lengths:                                      # short vectors: 16 slot classes, one element per thread, no pair loads
        LEN._assert_forms(n, T, dict(gy=16, per_dir=1, stream_trips=1, pair_loads=False))


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.HISTORY_UNSHARDED, ids=_id)
def test_lbfgs_iterations_at_a_full_history(case):
    n, T, history, iters = case
    _assert_case([n], T, history, iters)
    assert n > LEN.FIRST_SEGMENT and all(n % k for k in range(2, 33))              # prime: a ragged tail in every pass
    LEN._unsharded_run("stiff-" + _id(case), n, T, history, R.stiff_chain(n), iters)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.HISTORY_SHARDED, ids=_id)
def test_sharded_flow_at_a_full_history(case):
    lengths, T, history, iters = case
    _assert_case(lengths, T, history, iters)
    LEN._sharded_run(f"stiff-sharded-world{len(lengths)}-" + _id(case), list(lengths), T, history, R.stiff_chain(sum(lengths)), iters)


@pytest.mark.gpu
def test_fused_lbfgs_driver_at_a_full_history_replays_bit_for_bit():
    """optim.py's sequencing and segment offsets at a full ring, without a tolerance."""
    from hidenn_fem_amd.optim import FusedLBFGS
    c = R.HISTORY_FUSED
    n, n1, history, max_iter = c["n"], c["first_segment"], c["history"], c["max_iter"]
    dev = torch.device("cuda:0")
    prob = R.stiff_chain(n)
    a, b = torch.from_numpy(prob.a).to(dev), torch.from_numpy(prob.b).to(dev)
    x0 = torch.from_numpy(prob.x0.copy()).to(dev)
    params = [torch.nn.Parameter(x0[:n1].clone()), torch.nn.Parameter(x0[n1:].clone())]
    opt = FusedLBFGS(params, history_size=history, max_iter=max_iter, max_eval=10 ** 6)
    xs, gs, losses = [], [], []

    def closure():
        opt.zero_grad()
        x = torch.cat(params)
        dx = x[1:] - x[:-1]
        loss = 0.5 * ((a * x) @ x) + 0.5 * prob.c * (dx @ dx) - b @ x
        loss.backward()
        xs.append(x.detach().clone()), gs.append(torch.cat([p.grad for p in params]).clone()), losses.append(loss.item())
        return loss

    opt.step(closure)
    torch.cuda.synchronize()
    st_opt = opt.status()
    assert opt.state[params[0]]["n_iter"] == max_iter and len(xs) == max_iter
    assert (st_opt[R.ST_COUNT], st_opt[R.ST_FLAGS], st_opt[R.ST_NITER]) == (history, 0, max_iter - 1), st_opt

    H = LEN._Handle(n, history, F64)
    try:
        mine = [x0[:n1].clone(), x0[n1:].clone()]
        for k in range(max_iter):
            torch.cuda.synchronize()
            assert torch.equal(torch.cat(mine), xs[k]), (k, "the replayed parameters differ from the driver's")
            H.g.copy_(gs[k])
            H.loss.fill_(losses[k])
            st = H.check(after_update=k > 0)
            assert int(st[R.ST_FLAGS]) == 0 and st[R.ST_COUNT] == min(max(k - 1, 0), history), (k, st)
            H.direction()
            H.apply(mine)
        assert st == st_opt, (st, st_opt)
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(mine), torch.cat([p.detach() for p in params]))
        assert not torch.equal(torch.cat(mine), xs[-1])                           # the last iteration moved the parameters
    finally:
        H.close()
