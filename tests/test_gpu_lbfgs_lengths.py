"""The L-BFGS kernels (csrc/lbfgs.hip) at the vector lengths where their launch forms change, step by step through the C ABI
against tests/lbfgs_reference.py.  The rest of the suite stays below n = 39 000 and so only ever runs the small-n branch of:
  form 1   second grid-stride trip of gstats / pair / shard_pair (2048 blocks)            n > 524 288
  form 2   multidot with gy = clamp(2048 / nb_chunk, 1, 16) < 16 slot classes              n > 262 144; gy = 1 at n > 2 097 152
  form 3   fp32 multidot with 8 pair loads per thread (VEC = 2)                            fp32, n even, n >= 2^20
  form 3b  fp32, n >= 2^20 but odd: the scalar form                                        n = 1 048 577
  form 4   direction with 2 (fp64) / 4 (fp32) elements per thread                          n >= 2^20
  form 5   direction with 8 elements per thread                                            n >= 2 095 105
  form 6   second trip of apply / shard_apply / shard_gather (4096 blocks)                 a segment > 1 048 576 elements / rows
``_forms`` restates the host code that picks them; every case asserts the forms its id names before it runs.

Nothing but the kernels computes on the device: x lives there in T and ``apply`` updates it in place; after each apply it is
copied to the host, where ``ChainProblem`` (not taken from the code under test) gives loss and gradient in fp64, cast to T.
Both reference runs (float64, longdouble) get the direction and the step AS READ BACK FROM THE DEVICE, so their history has
the bits the kernels store.  Per iteration: the loss slot, max|g|, the flags, the count, n_iter and the parameters after apply
(given the device's own d and t) are compared bit for bit; g.d, t, H_diag and every element of d to ``R.allowed``: MARGIN x
the float64 run's own gap from the longdouble run + 64 eps (+ one fp32 ulp for an fp32 d), the error of d_i scaled by the
summed magnitudes of its terms |cg g_i| + sum_j (|cy_j Y_ji| + |cs_j S_ji|), that of g.d by sum_i |g_i| x that.

Schedule: history + 3 iterations (the ring wraps), one more check + direction whose apply is left out, check + direction
AGAIN on the same gradient (y = 0: the pair is rejected, new_slot = -1, the multidot pass takes its zero-load branch; d, count
and H_diag must stay), then a direction with tolerance_change = 1e30 (the g.d stop: the following apply leaves x bit-identical,
the next check reports bit 3).  Apply is called the way FusedLBFGS calls it for two parameter tensors: 37 elements, then the
rest.  The sharded flow: gather from permuted rows, local, finish, apply, at world = 1 and with two handles in one process
whose payloads are concatenated in rank order; one finish with want_direction = 0 (bit 4, nothing moves).

MEASURED on an MI355X (worst over a case's iterations of: the kernels' deviation / the float64 reference's own deviation, both
from the longdouble run, in units of the scales above; the file takes 40 s):
  unsharded        d                  g.d                t                  H_diag
  524289  fp64     6.2e-16 / 8.7e-16  2.2e-16 / 2.9e-16  1.4e-16 / 1.1e-16  2.1e-16 / 4.2e-16
  524289  fp32     5.9e-08 / 9.8e-16  2.1e-16 / 4.2e-16  5.1e-17 / 3.2e-16  3.2e-16 / 6.7e-16
  1048576 fp32     5.9e-08 / 1.1e-15  1.7e-16 / 3.3e-16  1.5e-16 / 2.2e-16  3.1e-16 / 8.5e-16
  1048576 fp64     8.0e-16 / 1.1e-15  1.4e-16 / 4.2e-16  1.7e-17 / 1.4e-16  3.7e-16 / 3.7e-16
  1048577 fp32     5.9e-08 / 1.1e-15  1.7e-16 / 3.9e-16  4.0e-17 / 3.3e-16  2.6e-16 / 7.5e-16
  1048577 fp64     5.2e-16 / 2.0e-15  1.5e-16 / 5.5e-16  4.3e-17 / 2.9e-16  1.8e-16 / 8.0e-16
  1048578 fp32     5.9e-08 / 2.7e-15  1.7e-16 / 6.2e-16  5.2e-17 / 2.0e-16  1.6e-16 / 9.6e-16
  2095104 fp64     6.9e-16 / 2.4e-15  1.7e-16 / 5.7e-16  2.8e-16 / 3.4e-16  2.3e-16 / 8.9e-16
  2095106 fp64     5.1e-16 / 1.8e-15  1.9e-16 / 4.9e-16  9.8e-17 / 4.0e-16  1.4e-16 / 1.0e-15
  2095106 fp32     6.0e-08 / 1.4e-15  2.4e-16 / 4.0e-16  8.4e-17 / 3.3e-16  2.7e-16 / 7.9e-16
  2097154 fp64     8.8e-16 / 1.6e-15  1.0e-16 / 5.6e-16  9.7e-19 / 3.7e-16  1.7e-16 / 1.0e-15
  2097154 fp32     5.9e-08 / 1.3e-15  1.4e-16 / 7.0e-16  2.0e-16 / 4.9e-17  2.7e-16 / 9.5e-16
  sharded, world 1
  1048578 fp64     4.7e-16 / 1.5e-15  1.4e-16 / 3.2e-16  6.6e-18 / 2.4e-16  1.3e-16 / 7.1e-16
  1048578 fp32     5.9e-08 / 2.7e-15  1.7e-16 / 6.2e-16  5.2e-17 / 2.0e-16  1.6e-16 / 9.6e-16
  2097154 fp64     8.8e-16 / 1.0e-15  1.0e-16 / 5.6e-16  9.7e-19 / 3.7e-16  1.7e-16 / 5.2e-16
  2097154 fp32     5.9e-08 / 1.3e-15  1.4e-16 / 7.0e-16  2.0e-16 / 4.9e-17  2.2e-16 / 7.4e-16
  524290  fp64     5.8e-16 / 9.0e-16  1.3e-16 / 3.9e-16  1.1e-16 / 2.6e-16  3.0e-16 / 5.6e-16
  1048576 fp32     5.9e-08 / 1.1e-15  1.7e-16 / 3.3e-16  1.5e-16 / 2.2e-16  3.1e-16 / 8.5e-16
  sharded, world 2 (1048578 + 4098)
  fp64             8.6e-16 / 1.6e-15  1.7e-16 / 5.2e-16  5.1e-17 / 2.0e-16  3.2e-16 / 8.2e-16
  fp32             5.9e-08 / 1.4e-15  1.5e-16 / 7.9e-16  1.1e-16 / 2.6e-16  3.3e-16 / 9.2e-16
The kernels (fp64 accumulation, tree-shaped sums) stay below the float64 reference's own gap everywhere; an fp32 d carries its
rounding to T (half an fp32 ulp, 5.96e-8) and nothing else.  MARGIN stays the 32 of ``cg_reference.allowed`` -- the kernels do
not need it; with it a case allows 3e-14 ... 1e-13 (fp32 d: 1.2e-7).  The smallest error any mutant of csrc/lbfgs.hip this
file was run against produced: 1.6e-7 in g.d where 2.2e-14 is allowed (one element left out of the sums at 524289)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lbfgs_reference as R

LR, TOL_GRAD, TOL_CHANGE = 1.0, 1e-7, 1e-9                 # torch.optim.LBFGS's defaults
MARGIN = 32.0
FIRST_SEGMENT = 37
K_LB, K_CHUNK = 256, 2048                                  # kLb, kLbChunk


def _forms(n, T):
    """The launch forms csrc/lbfgs.hip picks for a vector of n elements of type T (hfem_lbfgs_create / _direction / _apply)."""
    nb_chunk = -(-n // K_CHUNK)
    fp32 = T == np.float32
    return dict(stream_trips=-(-(-(-n // K_LB)) // 2048), gy=max(1, min(16, 2048 // nb_chunk)),
                pair_loads=bool(fp32 and n % 2 == 0 and n >= 1 << 20),
                per_dir=8 if nb_chunk >= 1024 else ((4 if fp32 else 2) if n >= 1 << 20 else 1),
                apply_trips=-(-(-(-(n - FIRST_SEGMENT) // K_LB)) // 4096), row_trips=-(-(-(-(n // 2) // K_LB)) // 4096))


F64, F32 = np.float64, np.float32
# (n, T, history, forms the id names)
LENGTHS = [
    (524289, F64, 8, dict(stream_trips=2, gy=7, per_dir=1)), (524289, F32, 8, dict(stream_trips=2, gy=7, per_dir=1, pair_loads=False)),
    (1048576, F32, 5, dict(pair_loads=True, per_dir=4, gy=4, apply_trips=1)), (1048576, F64, 5, dict(per_dir=2, gy=4, apply_trips=1)),
    (1048577, F32, 5, dict(pair_loads=False, per_dir=4, gy=3)), (1048577, F64, 5, dict(per_dir=2, gy=3)),
    (1048578, F32, 5, dict(pair_loads=True, per_dir=4, gy=3)),
    (2095104, F64, 5, dict(per_dir=2, gy=2)),
    (2095106, F64, 5, dict(per_dir=8, gy=2)), (2095106, F32, 5, dict(per_dir=8, gy=2, pair_loads=True)),
    (2097154, F64, 5, dict(per_dir=8, gy=1, apply_trips=2)), (2097154, F32, 5, dict(per_dir=8, gy=1, apply_trips=2, pair_loads=True)),
]


def _id(case):
    n, T, history, forms = case
    return f"n{n}-{'fp64' if T == F64 else 'fp32'}-h{history}-" + "-".join(f"{k}{int(v)}" for k, v in forms.items())


def _assert_forms(n, T, forms):
    have = _forms(n, T)
    assert {k: have[k] for k in forms} == forms, (n, T, have)


# ---------------------------------------------------------------------------------------------------------------- device side
class _DeviceArray:
    """A raw device pointer as something ``torch.as_tensor`` reads without a copy."""

    def __init__(self, ptr, n, T):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f8" if T == F64 else "<f4", data=(int(ptr), False), version=2)


class _Handle:
    """One ``hfem_lbfgs`` object and the device buffers a caller keeps beside it."""

    def __init__(self, n, history, T):
        from hidenn_fem_amd import _lib as B
        self.B, self.L, self.n, self.T = B, B.lib(), int(n), T
        self.dev = torch.device("cuda:0")
        self.tT = torch.float64 if T == F64 else torch.float32
        self.h = C.c_void_p()
        B.check(self.L.hfem_lbfgs_create(0, self.n, int(history), 0 if T == F64 else 1, C.byref(self.h)), "hfem_lbfgs_create")
        self.g = torch.zeros(self.n, dtype=self.tT, device=self.dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=self.dev)
        self.status = (C.c_double * 8)()
        self.stream = B.stream_ptr(self.dev)
        self._d = torch.as_tensor(_DeviceArray(self.L.hfem_lbfgs_direction_ptr(self.h), self.n, T), device=self.dev)
        assert self._d.dtype == self.tT and self._d.numel() == self.n

    def close(self):
        torch.cuda.synchronize()
        self._d = None
        self.L.hfem_lbfgs_destroy(self.h)
        self.h = None

    def upload(self, g, loss):
        self.g.copy_(torch.from_numpy(g))
        self.loss.fill_(float(loss))

    def check(self, after_update):
        self.B.check(self.L.hfem_lbfgs_check(self.h, self.g.data_ptr(), self.loss.data_ptr(), int(after_update), TOL_GRAD, TOL_CHANGE,
                                             self.status, self.stream), "hfem_lbfgs_check")
        return list(self.status)

    def direction(self, tolerance_change=TOL_CHANGE):
        self.B.check(self.L.hfem_lbfgs_direction(self.h, self.g.data_ptr(), LR, float(tolerance_change), self.stream),
                     "hfem_lbfgs_direction")
        return self.read_d()

    def apply(self, tensors):
        off = 0
        for p in tensors:
            self.B.check(self.L.hfem_lbfgs_apply(self.h, p.data_ptr(), off, p.numel(), self.stream), "hfem_lbfgs_apply")
            off += p.numel()
        assert off == self.n

    def read_d(self):
        torch.cuda.synchronize()
        return self._d.cpu().numpy().copy()


class _Shard(_Handle):
    """A handle of the sharded flow: the parameter rows it owns sit in two row arrays (x: nx rows, u: the rest; two values per
    row) in a random order; its flat local vector is [x rows rx | u rows ru]."""

    def __init__(self, n, history, T, seed):
        super().__init__(n, history, T)
        rows = n // 2
        self.nx = rows // 3
        self.nu = rows - self.nx
        rng = np.random.default_rng(seed)
        self.rx_h, self.ru_h = rng.permutation(self.nx).astype(np.int32), rng.permutation(self.nu).astype(np.int32)
        self.rx, self.ru = torch.from_numpy(self.rx_h).to(self.dev), torch.from_numpy(self.ru_h).to(self.dev)
        self.X = torch.zeros(self.nx, 2, dtype=self.tT, device=self.dev)
        self.U = torch.zeros(self.nu, 2, dtype=self.tT, device=self.dev)
        self.GX, self.GU = torch.zeros_like(self.X), torch.zeros_like(self.U)
        self.P = int(self.L.hfem_lbfgs_shard_payload_doubles(self.h))
        self.payload = torch.zeros(self.P, dtype=torch.float64, device=self.dev)

    def _to_rows(self, flat):
        X, U = np.empty((self.nx, 2), self.T), np.empty((self.nu, 2), self.T)
        X[self.rx_h], U[self.ru_h] = flat[:2 * self.nx].reshape(-1, 2), flat[2 * self.nx:].reshape(-1, 2)
        return X, U

    def set_parameters(self, flat):
        X, U = self._to_rows(flat)
        self.X.copy_(torch.from_numpy(X)), self.U.copy_(torch.from_numpy(U))

    def parameters(self):
        torch.cuda.synchronize()
        X, U = self.X.cpu().numpy(), self.U.cpu().numpy()
        return np.concatenate([X[self.rx_h].reshape(-1), U[self.ru_h].reshape(-1)])

    def gather(self, g_flat):
        """The gradient arrives in row arrays; the kernel under test makes the flat vector: it must be ``g_flat``'s bits."""
        X, U = self._to_rows(g_flat)
        self.GX.copy_(torch.from_numpy(X)), self.GU.copy_(torch.from_numpy(U))
        self.g.fill_(float("nan"))
        self.B.check(self.L.hfem_lbfgs_shard_gather(self.h, self.GX.data_ptr(), self.rx.data_ptr(), self.nx, self.GU.data_ptr(),
                                                    self.ru.data_ptr(), self.nu, self.g.data_ptr(), self.stream), "hfem_lbfgs_shard_gather")
        torch.cuda.synchronize()
        assert np.array_equal(self.g.cpu().numpy(), g_flat), "shard_gather"

    def local(self, loss):
        self.loss.fill_(float(loss))
        self.B.check(self.L.hfem_lbfgs_shard_local(self.h, self.g.data_ptr(), self.loss.data_ptr(), self.payload.data_ptr(), self.stream),
                     "hfem_lbfgs_shard_local")

    def finish(self, gathered, world, after_update, want_direction=True, tolerance_change=TOL_CHANGE):
        self.B.check(self.L.hfem_lbfgs_shard_finish(self.h, self.g.data_ptr(), gathered.data_ptr(), int(world), int(after_update),
                                                    int(want_direction), LR, TOL_GRAD, float(tolerance_change), self.status,
                                                    self.stream), "hfem_lbfgs_shard_finish")
        return list(self.status)

    def shard_apply(self):
        self.B.check(self.L.hfem_lbfgs_shard_apply(self.h, self.X.data_ptr(), self.rx.data_ptr(), self.nx, self.U.data_ptr(),
                                                   self.ru.data_ptr(), self.nu, self.stream), "hfem_lbfgs_shard_apply")


# ---------------------------------------------------------------------------------------------------------------- comparisons
class _Worst:
    """Worst scaled deviation per quantity over a case: the kernel's, and the float64 reference's own, from the longdouble run."""

    def __init__(self, name, T):
        self.name, self.T = name, T
        self.q = {k: [0.0, 0.0] for k in ("d", "gtd", "t", "H_diag")}

    def hold(self, what, got, ref64, refld, scale, extra=0.0, where=""):
        ld = np.longdouble
        dev = float((np.abs(np.asarray(ref64, dtype=ld) - refld) / scale).max())
        err = float((np.abs(np.asarray(got, dtype=ld) - refld) / scale).max())
        tol = R.allowed(dev, MARGIN) + extra
        print(f"LBFGS-LENGTHS {self.name} {where} {what}: kernel {err:.3e} reference {dev:.3e} allowed {tol:.3e}")
        self.q[what] = [max(self.q[what][0], err), max(self.q[what][1], dev)]
        assert err <= tol, (self.name, where, what, err, dev, tol)

    def report(self):
        print(f"LBFGS-LENGTHS-WORST {self.name} " + "  ".join(f"{k} {v[0]:.1e} / {v[1]:.1e}" for k, v in self.q.items()))


def _hold_direction(w, where, g, d_dev, r64, rld):
    """Every element of d, scaled by the summed magnitudes of its terms."""
    scale = np.maximum(r64.term_magnitudes(g), np.finfo(np.float64).tiny)
    w.hold("d", d_dev, r64.r, rld.r, scale, extra=R.EPS32 if w.T == F32 else 0.0, where=where)
    return float((np.abs(g.astype(np.float64)) * scale).sum())


def _hold_scalars(w, where, st, r64, rld, gtd_scale):
    """g.d, t, H_diag of the last direction, as a status record shows them."""
    w.hold("gtd", st[R.ST_GTD], r64.gtd, rld.gtd, gtd_scale, where=where)
    w.hold("t", st[R.ST_T], r64.t, rld.t, abs(rld.t), where=where)
    w.hold("H_diag", st[R.ST_HDIAG], r64.H_diag, rld.H_diag, abs(rld.H_diag), where=where)


def _assert_exact_slots(where, st, rec64, recld):
    for slot in (R.ST_LOSS, R.ST_FLAGS, R.ST_GMAX, R.ST_COUNT, R.ST_NITER):
        assert st[slot] == rec64[slot] == recld[slot], (where, "status slot", slot, st, rec64)


def _assert_applied(where, x_old, d, t, x_new):
    """x_new = T(double(x_old) + t double(d)) bit for bit: product and sum rounded separately, or -- every element then --
    contracted into one fused multiply-add."""
    if np.array_equal(x_new, R.apply_update(x_old, d, t)):
        return
    bad = np.nonzero(x_new != R.apply_update(x_old, d, t, fused=True))[0]
    assert bad.size <= 64, (where, "apply", bad.size, bad[:8])
    for i in bad:                                                                 # within ~1e-16 ulp of a tie: decided exactly
        assert x_new[i] == R.apply_update_exact(x_old[i], d[i], t), (where, "apply", int(i))


# ---------------------------------------------------------------------------------------------------------------- unsharded
def _unsharded_run(name, n, T, history, prob, iters):
    """The schedule of the module docstring with ``iters`` applied iterations on ``prob`` (tests/test_gpu_lbfgs_histories.py
    runs it too, on a problem that fills large histories)."""
    R.assert_longdouble_is_wider()
    w = _Worst(name, T)
    r64, rld = R.LbfgsReference(history, np.float64), R.LbfgsReference(history, np.longdouble)
    H = _Handle(n, history, T)
    try:
        x = prob.x0.astype(T)
        params = [torch.from_numpy(x[:FIRST_SEGMENT].copy()).to(H.dev), torch.from_numpy(x[FIRST_SEGMENT:].copy()).to(H.dev)]

        def read_x():
            torch.cuda.synchronize()
            return np.concatenate([p.cpu().numpy() for p in params])

        d_prev = t_prev = x_old = gtd_scale = None
        for k in range(iters + 3):
            # k < iters: check, direction, apply.  k = iters: no apply.  k = iters + 1: the same gradient again (rejected pair).
            # k = iters + 2: the same gradient, tolerance_change = 1e30 (the g.d stop), apply, one more check
            where = f"k={k}"
            if k <= iters:
                loss, g = prob.loss_and_grad(x)
                H.upload(g, loss)
            st = H.check(after_update=k > 0)
            if k > 0:
                t_prev = st[R.ST_T]                                   # the device's own step: the history's s = T(d t) needs its bits
                _hold_scalars(w, where, st, r64, rld, gtd_scale)
                if k <= iters:
                    _assert_applied(where, x_old, d_prev, t_prev, x)
            rec64, recld = (r.check(g, loss, d_prev, t_prev, after_update=k > 0) for r in (r64, rld))
            _assert_exact_slots(where, st, rec64, recld)
            if k <= iters:
                assert int(st[R.ST_FLAGS]) == 0, (where, st)           # the problem fires no break test
            else:
                assert int(st[R.ST_FLAGS]) == R.F_LOSS                 # the same evaluation twice: no loss change, nothing else
                if k == iters + 2:                                     # the rejected pair left count and H_diag alone, bit for bit
                    assert (st[R.ST_COUNT], st[R.ST_HDIAG]) == kept, (where, st, kept)
                kept = (st[R.ST_COUNT], st[R.ST_HDIAG])
            d_dev = H.direction(1e30 if k == iters + 2 else TOL_CHANGE)
            o64, old = (r.direction(g, d_prev, t_prev, 1e30 if k == iters + 2 else None) for r in (r64, rld))
            assert o64["accepted"] is old["accepted"] is (None if k == 0 else k <= iters), (where, o64["accepted"])
            assert o64["stop_gtd"] is old["stop_gtd"] is (k == iters + 2)
            gtd_scale = _hold_direction(w, where, g, d_dev, r64, rld)
            if k > iters:
                assert np.array_equal(d_dev, d_prev), (where, "a rejected pair changed the direction")
            d_prev = d_dev
            if k < iters or k == iters + 2:
                H.apply(params)
                x_old, x = x, read_x()
        assert np.array_equal(x, x_old), "apply after the g.d stop moved a parameter"
        st = H.check(after_update=1)
        rec64, recld = (r.check(g, loss, d_prev, st[R.ST_T]) for r in (r64, rld))
        _assert_exact_slots("after the stop", st, rec64, recld)
        assert int(st[R.ST_FLAGS]) == R.F_GTD | R.F_LOSS
        assert (st[R.ST_COUNT], st[R.ST_NITER]) == (history, iters + 3) and (st[R.ST_COUNT], st[R.ST_HDIAG]) == kept
        _hold_scalars(w, "after the stop", st, r64, rld, gtd_scale)
        w.report()
        return w
    finally:
        H.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", LENGTHS, ids=_id)
def test_lbfgs_iterations_at_a_length(case):
    n, T, history, forms = case
    _assert_forms(n, T, forms)
    _unsharded_run(_id(case), n, T, history, R.ChainProblem(n), history + 3)


# ---------------------------------------------------------------------------------------------------------------- sharded
def _sharded_run(name, lengths, T, history=5, prob=None, iters=None):
    """``len(lengths)`` handles in one process, nothing exchanged: their payloads concatenated in rank order go to every finish.
    The reference works on the whole vector [handle 0 | handle 1].  ``prob``: the ChainProblem of the summed length; ``iters``:
    history + 3 unless given."""
    R.assert_longdouble_is_wider()
    world, n = len(lengths), sum(lengths)
    w = _Worst(name, T)
    prob = R.ChainProblem(n) if prob is None else prob
    r64, rld = R.LbfgsReference(history, np.float64), R.LbfgsReference(history, np.longdouble)
    cuts = np.cumsum([0] + list(lengths))
    shards = []
    try:
        for r, nl in enumerate(lengths):
            shards.append(_Shard(nl, history, T, seed=100 + r))
        x = prob.x0.astype(T)
        for r, s in enumerate(shards):
            s.set_parameters(x[cuts[r]:cuts[r + 1]])

        def read_x():
            return np.concatenate([s.parameters() for s in shards])

        def finish_all(loss, g, **kw):
            for r, s in enumerate(shards):
                s.gather(g[cuts[r]:cuts[r + 1]])
                s.local(loss if r == 0 else 0.0)                      # the ranks' partial energies: summed in rank order
            gathered = shards[0].payload if world == 1 else torch.cat([s.payload for s in shards])
            sts = [s.finish(gathered, world, **kw) for s in shards]
            assert all(st == sts[0] for st in sts), ("the ranks' status records differ", sts)
            return sts[0], np.concatenate([s.read_d() for s in shards])

        assert np.array_equal(read_x(), x)
        d_prev = t_prev = None
        iters = history + 3 if iters is None else iters
        skip_at = 3                                                   # before this iteration: one finish with want_direction = 0
        for k in range(iters + 1):
            where = f"k={k}"
            last = k == iters                                         # the same gradient, after_update = 0, tolerance_change = 1e30
            if not last:
                loss, g = prob.loss_and_grad(x)
            if k == skip_at:
                st, d_dev = finish_all(loss, g, after_update=1, want_direction=False)
                o64, old = (r.shard_iterate(g, loss, d_prev, t_prev, want_direction=False) for r in (r64, rld))
                _assert_exact_slots(where + " skipped", st, o64["status"], old["status"])
                assert int(st[R.ST_FLAGS]) == R.F_NODIR and st[3:] == st_prev[3:], (st, st_prev)
                assert np.array_equal(d_dev, d_prev)
                for s in shards:
                    s.shard_apply()
                assert np.array_equal(read_x(), x), "apply after a finish without a direction moved a parameter"
            # (a finish that computed no direction ends the caller's step: the device ignores after_update = 1 iterations
            # behind it -- LbfgsState.halt, for several iterations per graph -- until the next step opens with after_update = 0)
            kw = dict(after_update=0, tolerance_change=1e30) if last else dict(after_update=int(k > 0 and k != skip_at))
            st, d_dev = finish_all(loss, g, **kw)
            o64, old = (r.shard_iterate(g, loss, d_prev, t_prev, after_update=bool(kw["after_update"]),
                                        tolerance_change=kw.get("tolerance_change")) for r in (r64, rld))
            _assert_exact_slots(where, st, o64["status"], old["status"])
            assert int(st[R.ST_FLAGS]) == (R.F_GTD if last else 0), (where, st)
            assert o64["accepted"] is old["accepted"] is (None if k == 0 else not last)
            gtd_scale = _hold_direction(w, where, g, d_dev, r64, rld)
            _hold_scalars(w, where, st, r64, rld, gtd_scale)
            if last:
                assert np.array_equal(d_dev, d_prev), "a rejected pair changed the direction"
            d_prev, t_prev, st_prev = d_dev, st[R.ST_T], st
            for s in shards:
                s.shard_apply()
            x_old, x = x, read_x()
            if last:
                assert np.array_equal(x, x_old), "apply after the g.d stop moved a parameter"
            else:
                _assert_applied(where, x_old, d_prev, t_prev, x)
        assert (st[R.ST_COUNT], st[R.ST_NITER]) == (history, iters + 1)
        w.report()
        return w
    finally:
        for s in shards:
            s.close()


# The issue's two lengths in both types, and two more: the speculative pair makes the multidot pass take count + 1 slots, so with
# gy = 7 and history 8 (gy = 4 and history 5) a slot class has a second slot that no neighbouring class reaches.  The unsharded
# runs at these gy have at most gy + 1 slots and are blind to a slot loop that steps by 1 instead of gy: class c + 1 computes
# the same value for the slot class c takes by mistake, and class gy - 1 reaches the last one.
SHARDED = [
    (1048578, F64, 5, dict(gy=3, per_dir=2, row_trips=1)), (1048578, F32, 5, dict(gy=3, per_dir=4, row_trips=1, pair_loads=True)),
    (2097154, F64, 5, dict(gy=1, per_dir=8, row_trips=2)), (2097154, F32, 5, dict(gy=1, per_dir=8, row_trips=2, pair_loads=True)),
    (524290, F64, 8, dict(gy=7, per_dir=1, stream_trips=2)), (1048576, F32, 5, dict(gy=4, per_dir=4, pair_loads=True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHARDED, ids=_id)
def test_sharded_flow_one_rank_at_a_length(case):
    n, T, history, forms = case
    _assert_forms(n, T, forms)
    _sharded_run("sharded-world1-" + _id(case), [n], T, history)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [F64, F32], ids=["fp64", "fp32"])
def test_sharded_flow_two_handles_share_one_decision(T):
    _assert_forms(1048578, T, dict(gy=3, stream_trips=3))
    _assert_forms(4098, T, dict(gy=16, per_dir=1, stream_trips=1, pair_loads=False))
    _sharded_run(f"sharded-world2-n1048578+4098-{'fp64' if T == F64 else 'fp32'}", [1048578, 4098], T)
