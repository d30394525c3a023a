"""The Adam kernels of csrc/optim.hip at the edges of their launch forms, against the formula (tests/adam_cases.py: ``adam_numpy``
and ``adam_longdouble``; the cases and bounds are pinned by tests/test_adam_cases_host.py).  Every call goes through the C ABI
except F:

  A  ``hfem_adam_step`` and ``hfem_adam_step_dev`` (its counter advanced by ``hfem_counter_add``), fp64 and fp32: lengths around
     one vector and one block, the grid cap of 2048 blocks exactly and one trip more; n = 0; views offset by one element (all
     four arrays, g alone, v alone), fp32 by two -- the scalar loop, once through its second trip
  B  ``hfem_adam_step_rows2_dev`` and ``_f32``: the x/u split inside a block and at its edge, n_x = 0, n_u = 0, two learning
     rates, step_offset 0 and 1, unlisted rows bit-identical; the hand-written fp64 statement against ``adam_one`` (A's kernel)
  C  ``hfem_adam_multi_dev`` on tables built by hand: chunk_vecs 1 .. 512 on seven tensors (a tail, no vector, n = 0, fp32, an
     unaligned view with an idle second block, other betas, exactly one chunk), 40 one-block tensors, idle blocks, 6000 blocks,
     the ticket counter's regimes (the step counter grows by one and the tickets are back at zero after EVERY launch), the
     host-step form, and ``FusedAdam._table``'s layout at chunk 512
  D  refused calls (argument checks only: each returns before any launch)
  E  special values (zero gradient, g*g overflowing and underflowing, step 10^6, beta1 = 0, eps = 0) and ``hfem_adam_prep``
  F  ``FusedAdam`` where it takes the launches no other test reaches: one tensor, diverging step counts, offset views

Data never cancels (|p| >= 0.5, gradients and moments of one sign per entry), so every bound is RELATIVE AND PER ENTRY.  fp64:
``ADAM_RTOL`` = 1e-14 against ``adam_numpy``.  fp32: against ``adam_longdouble``, 4 x the error ``adam_numpy`` in fp32 itself shows
against it on 200 000 such entries over the same steps (``adam_cases.fp32_allowance``; 3 steps: p 6.7e-7, m 5.9e-7, v 1.3e-6).
Buffers carry NaN guards behind the payload and in front of it, the two elements next to the payload being finite sentinels (an
in-place update of a NaN would go unseen); all of them must be unchanged after the call.

Measured on an MI355X (every test prints its figures under ``-s``): in fp64 the worst entry of any test sits at 0.066 of
ADAM_RTOL; in fp32 the worst error over allowance is 0.252 (p at 2 098 179 entries: 1.18e-7, exactly ``adam_numpy``'s own error
there -- the kernel is no further from longdouble than the restatement is, and 148 of its 555 compared arrays equal
``adam_numpy``'s bit for bit); ``FusedAdam`` against ``torch.optim.Adam`` on the GPU: at most 0.195 of the bounds.  Aligned and offset
calls gave the same bits in every case, so did ``hfem_adam_step_rows2_dev`` and ``adam_one``; ``hfem_adam_prep`` was 0 ulp off.
The whole file (116 tests) takes 6 s, the slowest test 1.7 s (``FusedAdam`` on 1 048 578 entries).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as A
from test_gpu_pointwise_edges import Abi, close

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
FRONT, GUARD = 8, 64                                    # elements in front of (a multiple of 16 bytes) and behind a payload
SENTINEL = dict(p=1.0, g=2.0, m=0.5, v=0.25)            # an update of such an entry would change p, m and v
DT = {F64: 0, F32: 1}
ENTRIES = ("hfem_adam_step", "hfem_adam_step_dev")


class Buf:
    """``data`` (numpy) on the device, ``offset`` elements past a 16-byte boundary, inside one guarded allocation."""

    def __init__(self, data, d, kind="p", offset=0):
        data = np.ascontiguousarray(data).reshape(-1)
        self.n, self.lo = data.size, FRONT + offset
        self.t = torch.full((self.lo + self.n + GUARD,), NAN, dtype=torch.from_numpy(data[:0].copy()).dtype, device=d)
        self.t[self.lo - 1] = self.t[self.lo + self.n] = SENTINEL[kind]
        self.view = self.t[self.lo:self.lo + self.n]
        self.set(data)
        assert self.t.data_ptr() % 16 == 0 and (self.ptr % 16 == 0) == (offset * data.itemsize % 16 == 0)
        self.frame = self._frame()

    def set(self, data):
        self.view.copy_(torch.from_numpy(np.array(data).reshape(-1)))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def _frame(self):
        bits = self.t.view(torch.int64 if self.t.dtype == F64 else torch.int32)
        return torch.cat([bits[:self.lo], bits[self.lo + self.n:]]).cpu()

    def get(self, what):
        """The payload as numpy; everything around it must be unchanged bit for bit."""
        assert torch.equal(self._frame(), self.frame), f"{what}: wrote outside its payload"
        return self.view.cpu().numpy()


def hyper_args(h):
    return h["lr"], h["beta1"], h["beta2"], h["eps"]


def allowance(dtype, steps, zero_state=False, hyper=A.HYPER):
    return A.fp32_allowance(steps, zero_state, hyper) if dtype == F32 else None


def held(got, ref, ld, dtype, allow, what, init=None):
    """got / ref / ld: (p, m, v).  fp64: ADAM_RTOL per entry against adam_numpy; fp32: ``allow`` per entry against longdouble."""
    for i, name in enumerate("pmv"):
        g = np.asarray(got[i]).reshape(-1)
        assert np.isfinite(g).all(), f"{what} {name}"
        if dtype == F64:
            close(torch.from_numpy(g.copy()), torch.from_numpy(np.array(ref[i]).reshape(-1)), A.ADAM_RTOL, 0.0, f"{what} {name}")
        else:
            assert g.dtype == np.float32
            err, own = A.rel_err(g, ld[i]), A.rel_err(ref[i], ld[i])
            print(f"{what} {name}: err {err:.3e}, err / allowance {err / allow[name]:.3f}, adam_numpy's own {own:.3e}, "
                  f"bitwise adam_numpy: {np.array_equal(g, np.asarray(ref[i]).reshape(-1))}")
            assert err <= allow[name], f"{what} {name}: err / allowance {err / allow[name]:.3f}"
        if init is not None and g.size:
            assert (g != np.asarray(init[i]).reshape(-1)).all(), f"{what} {name}: an entry was not updated"


# ------------------------------------------------------------------------------------------------ A: the flat kernels
def run_flat(a, entry, dtype, d, steps, hyper, offsets=(0, 0, 0, 0), first_step=1):
    """``steps`` launches of ``entry`` on adam_data ``d`` -> (p, m, v) as numpy, guards checked."""
    n = d["p"].size
    b = {k: Buf(d[k] if k != "g" else d["grads"][0], a.d, k, off) for k, off in zip("pgmv", offsets)}
    counter = torch.full((1,), first_step - 1, dtype=torch.int64, device=a.d)
    for k in range(steps):
        b["g"].set(d["grads"][k])
        if entry == "hfem_adam_step":
            a.ok(a.L.hfem_adam_step(a.di, b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, n, DT[dtype], *hyper_args(hyper),
                                    first_step + k, a.st), entry)
        else:
            a.ok(a.L.hfem_counter_add(a.di, a.ptr(counter), 1, a.st), "hfem_counter_add")
            a.ok(a.L.hfem_adam_step_dev(a.di, b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, n, DT[dtype], *hyper_args(hyper),
                                        a.ptr(counter), a.st), entry)
            torch.cuda.synchronize()
            assert counter.item() == first_step + k
    torch.cuda.synchronize()
    b["g"].get("g")
    return tuple(b[k].get(f"{entry} {k}") for k in "pmv")


def init_of(d):
    return d["p"], d["m"], d["v"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("dtype,n", [(dt, n) for dt in (F64, F32) for n in A.LENGTHS[dt]], ids=lambda x: str(x).replace("torch.", ""))
def test_flat_lengths(dtype, n, entry):
    """A: every length; the lengths from the grid cap on run 2 steps."""
    a, steps = Abi(), A.steps_of(n, dtype)
    d, ref, ld = A.reference(n, dtype, 100 + n % 97, steps)
    got = run_flat(a, entry, dtype, d, steps, A.HYPER)
    held(got, ref[-1], ld and ld[-1], dtype, allowance(dtype, steps), f"A {entry} n={n}", init_of(d))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_flat_empty_call_needs_no_pointer(dtype):
    a = Abi()
    step = torch.ones(1, dtype=torch.int64, device=a.d)
    assert a.L.hfem_adam_step(a.di, None, None, None, None, 0, DT[dtype], *hyper_args(A.HYPER), 1, a.st) == 0
    assert a.L.hfem_adam_step_dev(a.di, None, None, None, None, 0, DT[dtype], *hyper_args(A.HYPER), None, a.st) == 0
    torch.cuda.synchronize()
    assert step.item() == 1


OFFSETS = {"all four by one": (1, 1, 1, 1), "g alone": (0, 1, 0, 0), "v alone": (0, 0, 0, 1)}


OFFSET_CASES = [(dt, w) for dt in (F64, F32) for w in OFFSETS] + [(F32, "all four by two")]   # two fp64 elements: an aligned view


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("dtype,which", OFFSET_CASES, ids=lambda x: str(x).replace("torch.", "").replace(" ", "_"))
def test_flat_offset_views(dtype, which, entry):
    """A: views that do not start on a 16-byte boundary take the scalar loop; the entries around them stay as they were.
    Whether the aligned call gives the same bits is printed, not asserted (both run adam_one)."""
    offsets = OFFSETS.get(which, (2, 2, 2, 2))
    a, n = Abi(), A.OFFSET_N[dtype]
    d, ref, ld = A.reference(n, dtype, 131, A.STEPS)
    got = run_flat(a, entry, dtype, d, A.STEPS, A.HYPER, offsets)
    held(got, ref[-1], ld and ld[-1], dtype, allowance(dtype, A.STEPS), f"A {entry} offset {which}", init_of(d))
    aligned = run_flat(a, entry, dtype, d, A.STEPS, A.HYPER)
    print(f"A {entry} {dtype} offset {which}: bitwise equal to the aligned call: {all(np.array_equal(x, y) for x, y in zip(got, aligned))}")


def test_flat_offset_view_second_trip_of_the_scalar_loop():
    """A: 1 049 089 fp64 entries, all four arrays offset by one element: 2048 blocks x 256 threads, three trips."""
    a, n = Abi(), A.ONE_TRIP_MORE[F64]
    assert A.vector_trips(n, F64, aligned=False) >= 2
    d, ref, _ = A.reference(n, F64, 100 + n % 97, A.BIG_STEPS)
    got = run_flat(a, "hfem_adam_step", F64, d, A.BIG_STEPS, A.HYPER, (1, 1, 1, 1))
    held(got, ref[-1], None, F64, None, "A offset n=1049089", init_of(d))


# ------------------------------------------------------------------------------------------------ B: listed rows of two tensors
def run_rows2(a, dtype, c, n_x, n_u, steps, step_offset, lr_x=A.LR_X, lr_u=A.LR_U):
    entry = a.L.hfem_adam_step_rows2_dev if dtype == F64 else a.L.hfem_adam_step_rows2_dev_f32
    bx = {k: Buf(c["x"][k] if k != "g" else c["x"]["grads"][0], a.d, k) for k in "pgmv"}
    bu = {k: Buf(c["u"][k] if k != "g" else c["u"]["grads"][0], a.d, k) for k in "pgmv"}
    rx, ru = c["rows_x"].to(a.d), c["rows_u"].to(a.d)
    px = lambda bufs, n: [bufs[k].ptr if n else None for k in "pgmv"]
    counter = torch.zeros(1, dtype=torch.int64, device=a.d)
    h = A.HYPER
    for k in range(steps):
        bx["g"].set(c["x"]["grads"][k])
        bu["g"].set(c["u"]["grads"][k])
        if step_offset == 0:                                # the counter bumped before the launch ...
            a.ok(a.L.hfem_counter_add(a.di, a.ptr(counter), 1, a.st), "hfem_counter_add")
        a.ok(entry(a.di, *px(bx, n_x), a.ptr(rx) if n_x else None, n_x, lr_x, *px(bu, n_u), a.ptr(ru) if n_u else None, n_u, lr_u,
                   h["beta1"], h["beta2"], h["eps"], a.ptr(counter), step_offset, a.st), "hfem_adam_step_rows2_dev")
        if step_offset == 1:                                # ... or one behind, and bumped after it
            a.ok(a.L.hfem_counter_add(a.di, a.ptr(counter), 1, a.st), "hfem_counter_add")
        torch.cuda.synchronize()
        assert counter.item() == k + 1
    return {k: bx[k].get(f"x {k}").reshape(-1, 2) for k in "pmv"}, {k: bu[k].get(f"u {k}").reshape(-1, 2) for k in "pmv"}


def rows_held(got, d, rows, lr, dtype, steps, what):
    n_rows = d["p"].size // 2
    listed = np.zeros(n_rows, dtype=bool)
    listed[rows.numpy()] = True
    for k in "pmv":
        assert np.array_equal(got[k][~listed].view(np.uint8), d[k].reshape(-1, 2)[~listed].view(np.uint8)), f"{what} {k}: an unlisted row changed"
    if not len(rows):
        return
    r = rows.long().numpy()
    ref = A.rows_expected(d, r, steps, lr, dtype)[-1]
    ld = A.rows_expected(d, r, steps, lr, dtype, ld=True)[-1] if dtype == F32 else None
    init = tuple(d[k].reshape(-1, 2)[r] for k in "pmv")
    held(tuple(got[k][r] for k in "pmv"), ref, ld, dtype, allowance(dtype, steps, False, dict(A.HYPER, lr=lr)), what, init)


@pytest.mark.parametrize("step_offset", [0, 1])
@pytest.mark.parametrize("n_x,n_u", A.ROW_SPLITS)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_rows2_splits_rates_and_step_offset(dtype, n_x, n_u, step_offset):
    """B: the same reference steps 1, 2, 3 whether the counter is bumped before (offset 0) or after (offset 1) the launch."""
    a, c = Abi(), A.rows2_case(n_x, n_u, dtype)
    gx, gu = run_rows2(a, dtype, c, n_x, n_u, A.STEPS, step_offset)
    rows_held(gx, c["x"], c["rows_x"], A.LR_X, dtype, A.STEPS, f"B {dtype} ({n_x},{n_u}) offset {step_offset} x")
    rows_held(gu, c["u"], c["rows_u"], A.LR_U, dtype, A.STEPS, f"B {dtype} ({n_x},{n_u}) offset {step_offset} u")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_rows2_empty_call_needs_no_pointer(dtype):
    a = Abi()
    entry = a.L.hfem_adam_step_rows2_dev if dtype == F64 else a.L.hfem_adam_step_rows2_dev_f32
    assert entry(a.di, None, None, None, None, None, 0, A.LR_X, None, None, None, None, None, 0, A.LR_U, 0.9, 0.999, 1e-8, None, 0, a.st) == 0


def test_rows2_fp64_statement_is_adam_one():
    """B: hfem_adam_step_rows2_dev restates the update by hand; hfem_adam_step_dev on the same rows gathered into a dense tensor
    runs adam_one<double>.  Both within ADAM_RTOL of the reference (whether they agree to the bit is printed)."""
    a, (n_x, n_u) = Abi(), A.ROW_SPLITS[0]
    c = A.rows2_case(n_x, n_u, F64)
    gx, gu = run_rows2(a, F64, c, n_x, n_u, A.STEPS, 0)
    for got, d, rows, lr, tag in ((gx, c["x"], c["rows_x"], A.LR_X, "x"), (gu, c["u"], c["rows_u"], A.LR_U, "u")):
        r = rows.long().numpy()
        dense = dict(p=d["p"].reshape(-1, 2)[r].reshape(-1), m=d["m"].reshape(-1, 2)[r].reshape(-1), v=d["v"].reshape(-1, 2)[r].reshape(-1),
                     grads=[g.reshape(-1, 2)[r].reshape(-1) for g in d["grads"]])
        flat = run_flat(a, "hfem_adam_step_dev", F64, dense, A.STEPS, dict(A.HYPER, lr=lr))
        ref = A.rows_expected(d, r, A.STEPS, lr, F64)[-1]
        held(flat, ref, None, F64, None, f"B adam_one {tag}", init_of(dense))
        held(tuple(got[k][r] for k in "pmv"), ref, None, F64, None, f"B rows2 {tag}")
        print(f"B rows2 against adam_one, {tag}: bitwise equal {all(np.array_equal(got[k][r].reshape(-1), f) for k, f in zip('pmv', flat))}")


# ------------------------------------------------------------------------------------------------ C: the multi-tensor kernel
class Table:
    """A device table of ``tensors`` ((n, dtype, hyper, offset, blocks) as adam_cases.seven_tensors gives them) with their
    guarded buffers and references."""

    def __init__(self, a, tensors, chunk, steps=A.STEPS, seed=500, first_step=1):
        from hidenn_fem_amd import _lib
        self.a, self.tensors, self.chunk, self.steps = a, tensors, chunk, steps
        self.begin, self.need = A.table_layout(tensors, chunk)
        self.refs = [A.reference(n, dt, seed + i, steps, hyper=h, first_step=first_step) for i, (n, dt, h, _, _) in enumerate(tensors)]
        self.bufs = []
        tab = (_lib.AdamTensor * len(tensors))()
        for e, (n, dt, h, off, _), (d, _, _), b0 in zip(tab, tensors, self.refs, self.begin):
            src = d if n else dict(p=np.full(4, NAN, A.NP[dt]), m=np.full(4, NAN, A.NP[dt]), v=np.full(4, NAN, A.NP[dt]),
                                   grads=[np.full(4, NAN, A.NP[dt])])     # n = 0: pointers to memory that must stay as it is
            b = {k: Buf(src[k] if k != "g" else src["grads"][0], a.d, k, off) for k in "pgmv"}
            self.bufs.append(b)
            e.p, e.g, e.m, e.v, e.n = b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, n
            e.lr, e.beta1, e.beta2, e.eps = hyper_args(h)
            e.dtype, e.block_begin = DT[dt], b0
        self.dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(a.d)
        self.step_dev = torch.full((1,), first_step - 1, dtype=torch.int64, device=a.d)
        self.ticket = torch.zeros(_lib.ADAM_TICKET_INTS + GUARD, dtype=torch.int32, device=a.d)
        self.ticket[_lib.ADAM_TICKET_INTS:] = 77
        self.ints = _lib.ADAM_TICKET_INTS

    def set_grads(self, k):
        for b, (n, *_), (d, _, _) in zip(self.bufs, self.tensors, self.refs):
            if n:
                b["g"].set(d["grads"][k])

    def launch(self, n_blocks, device_step=True, step_offset=1):
        a = self.a
        a.ok(a.L.hfem_adam_multi_dev(a.di, a.ptr(self.dev), len(self.tensors), n_blocks, self.chunk,
                                     a.ptr(self.step_dev) if device_step else None, step_offset,
                                     a.ptr(self.ticket) if device_step else None, a.st), "hfem_adam_multi_dev")
        torch.cuda.synchronize()

    def tickets_are_zero(self):
        t = self.ticket.cpu()
        assert not t[:self.ints].any(), f"tickets left: {t[:self.ints].nonzero().reshape(-1).tolist()}"
        assert (t[self.ints:] == 77).all(), "wrote past the ticket buffer"

    def held(self, k, what):
        """Every tensor after step k + 1 (0-based k)."""
        for i, (b, (n, dt, h, off, _), (d, ref, ld)) in enumerate(zip(self.bufs, self.tensors, self.refs)):
            got = tuple(b[name].get(f"{what} tensor {i} {name}") for name in "pmv")
            b["g"].get(f"{what} tensor {i} g")
            if not n:
                assert all(np.isnan(g).all() for g in got)
                continue
            held(got, ref[k], ld and ld[k], dt, allowance(dt, self.steps, False, h), f"{what} tensor {i} step {k + 1}",
                 init_of(d) if k == 0 else ref[k - 1])


def run_table(tab, n_blocks, what):
    for k in range(tab.steps):
        tab.set_grads(k)
        tab.launch(n_blocks)
        assert tab.step_dev.item() == k + 1, f"{what}: the step counter after launch {k + 1}"
        tab.tickets_are_zero()
        tab.held(k, what)


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("chunk", A.CHUNKS)
def test_multi_seven_tensors(chunk, extra):
    """C: every chunk size, n_blocks the table's need and 5 more (idle blocks must do nothing but take their tickets)."""
    tab = Table(Abi(), A.seven_tensors(chunk), chunk)
    run_table(tab, tab.need + extra, f"C chunk {chunk} +{extra}")


def test_multi_forty_one_block_tensors():
    """C: the table scan over 40 entries; lengths 1 .. 50, both dtypes, three learning rates."""
    tensors = [(1 + (7 * i) % 50, (F64, F32)[i % 2], dict(A.HYPER, lr=(1e-2, 9e-3, 7e-3)[i // 2 % 3]), 0, None) for i in range(40)]
    tab = Table(Abi(), tensors, 256, seed=700)
    assert tab.need == 40
    run_table(tab, 40, "C forty")


def test_multi_more_blocks_than_the_device_holds():
    """C: chunk_vecs = 1 on 6000 vectors + 1 element: 6000 blocks, the later ones start after the first have finished -- a
    tail that every block applied would be seen here whatever the timing."""
    tab = Table(Abi(), [(2 * A.MANY_BLOCKS + 1, F64, A.HYPER, 0, None)], 1, seed=800)
    assert tab.need == A.MANY_BLOCKS
    run_table(tab, tab.need, "C 6000 blocks")


@pytest.mark.parametrize("n_blocks", A.TICKET_BLOCKS)
def test_multi_ticket_regimes(n_blocks):
    """C: one fp64 tensor, chunk_vecs = 1, n = 2 n_blocks; fewer blocks than ticket classes, exactly 32, more and no multiple.
    After each of three launches on ONE ticket buffer: the counter grew by exactly 1, all HFEM_ADAM_TICKET_INTS are 0, and the
    update was the reference's step 1, 2, 3."""
    tab = Table(Abi(), [(2 * n_blocks, F64, A.HYPER, 0, None)], 1, seed=900)
    assert tab.need == n_blocks
    run_table(tab, n_blocks, f"C tickets {n_blocks}")


def test_multi_host_step_form():
    """C: step_dev = NULL, ticket = NULL, step_offset = k is the reference's step k; nothing touches a counter."""
    tab = Table(Abi(), A.seven_tensors(300), 300, first_step=4)
    for k in range(tab.steps):
        tab.set_grads(k)
        tab.launch(tab.need, device_step=False, step_offset=4 + k)
        assert tab.step_dev.item() == 3
        tab.tickets_are_zero()
        tab.held(k, f"C host step {4 + k}")


def test_fused_adam_table_layout_at_chunk_512():
    """C: ``FusedAdam._table`` at a size that gives chunk 512 (the in-chunk loop's second trip through the Python path):
    blocks, chunk and every block_begin against a plain restatement, the update against the formula."""
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.optim import FusedAdam
    a, steps = Abi(), A.BIG_STEPS
    numels, dtypes = [1_048_578, 37], [F64, F32]
    refs = [A.reference(n, dt, 40 + i, steps, zero_state=True) for i, (n, dt) in enumerate(zip(numels, dtypes))]
    params = [torch.nn.Parameter(torch.from_numpy(d["p"].copy()).to(a.d)) for d, _, _ in refs]
    opt = FusedAdam(params, **{"lr": A.HYPER["lr"], "betas": (A.HYPER["beta1"], A.HYPER["beta2"]), "eps": A.HYPER["eps"]}, capturable=True)
    for k in range(steps):
        for p, (d, _, _) in zip(params, refs):
            p.grad = torch.from_numpy(d["grads"][k].copy()).to(a.d)
        opt.step()
    torch.cuda.synchronize()
    assert opt._step_dev.item() == steps and not opt._ticket.any()
    chunk, begin, blocks = A.fused_table_layout(numels, dtypes)
    used = [sl for sl in opt._tabs["slots"] if sl["key"] is not None]
    assert used and chunk == 512
    for sl in used:
        _, n, got_blocks, got_chunk, _ = sl["entry"]
        tab = (_lib.AdamTensor * n).from_buffer_copy(bytes(sl["host"][:n * C.sizeof(_lib.AdamTensor)].numpy()))
        assert (n, got_blocks, got_chunk) == (2, blocks, chunk) and [e.block_begin for e in tab] == begin
        assert [e.n for e in tab] == numels and [e.dtype for e in tab] == [0, 1]
    for i, (p, (d, ref, ld)) in enumerate(zip(params, refs)):
        st = opt.state[p]
        got = tuple(t.detach().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))
        held(got, ref[-1], ld and ld[-1], dtypes[i], allowance(dtypes[i], steps, True), f"C FusedAdam table tensor {i}")


# ------------------------------------------------------------------------------------------------ D: refused calls
def test_refused_calls_name_their_entry_point_and_launch_nothing():
    """D: argument checks only -- every call below returns before any launch; the buffers are as they were."""
    from hidenn_fem_amd import _lib
    a, h = Abi(), hyper_args(A.HYPER)
    d = A.adam_data(16, F64, 3)
    b = {k: Buf(d[k] if k != "g" else d["grads"][0], a.d, k) for k in "pgmv"}
    P = [b[k].ptr for k in "pgmv"]
    rows = torch.arange(4, dtype=torch.int32, device=a.d)
    step = torch.ones(1, dtype=torch.int64, device=a.d)
    bc = torch.zeros(2, dtype=F64, device=a.d)
    ticket = torch.zeros(_lib.ADAM_TICKET_INTS, dtype=torch.int32, device=a.d)
    L, R, S = a.L, a.ptr(rows), a.ptr(step)
    for dt in (0, 1):
        a.refused(L.hfem_adam_step(a.di, *P, -1, dt, *h, 1, a.st), b"hfem_adam_step:", b"need n >= 0 and step >= 1")
        a.refused(L.hfem_adam_step(a.di, *P, 8, dt, *h, 0, a.st), b"hfem_adam_step:", b"need n >= 0 and step >= 1")
        a.refused(L.hfem_adam_step_dev(a.di, *P, -1, dt, *h, S, a.st), b"hfem_adam_step_dev:", b"need n >= 0")
    a.refused(L.hfem_adam_step(a.di, *P, 8, 2, *h, 1, a.st), b"hfem_adam_step:", b"dtype: 0 = fp64, 1 = fp32")
    a.refused(L.hfem_adam_step_dev(a.di, *P, 8, 2, *h, S, a.st), b"hfem_adam_step_dev:", b"dtype: 0 = fp64, 1 = fp32")
    nulled = lambda args, i: [None if j == i else x for j, x in enumerate(args)]
    for i in range(4):
        a.refused(L.hfem_adam_step(a.di, *nulled(P, i), 8, 0, *h, 1, a.st), b"hfem_adam_step:", b"null pointer")
    for i in range(5):
        q = nulled(P + [S], i)
        a.refused(L.hfem_adam_step_dev(a.di, *q[:4], 8, 0, *h, q[4], a.st), b"hfem_adam_step_dev:", b"null pointer")
    for i in range(6):
        q = nulled(P + [R, S], i)
        a.refused(L.hfem_adam_step_rows_dev(a.di, *q[:5], 4, *h, q[5], a.st), b"hfem_adam_step_rows_dev:", b"null pointer")
    a.refused(L.hfem_adam_step_rows_dev(a.di, *P, R, -1, *h, S, a.st), b"hfem_adam_step_rows_dev:", b"negative row count")
    for name in ("hfem_adam_step_rows2_dev", "hfem_adam_step_rows2_dev_f32"):
        fn, full = getattr(L, name), P + [R] + P + [R] + [S]
        call = lambda q, nx, nu: fn(a.di, *q[:5], nx, A.LR_X, *q[5:10], nu, A.LR_U, h[1], h[2], h[3], q[10], 0, a.st)
        for i in range(11):
            a.refused(call(nulled(full, i), 4, 4), name.encode() + b":", b"null pointer")
        a.refused(call(nulled(full, 10), 4, 0), name.encode() + b":", b"null pointer")           # the counter, whichever half is empty
        a.refused(call(nulled(full, 10), 0, 4), name.encode() + b":", b"null pointer")
        a.refused(call(full, -1, 4), name.encode() + b":", b"negative row count")
        a.refused(call(full, 4, -1), name.encode() + b":", b"negative row count")
    tab = torch.zeros(C.sizeof(_lib.AdamTensor), dtype=torch.uint8, device=a.d)
    T, K = a.ptr(tab), a.ptr(ticket)
    M = b"hfem_adam_multi_dev:"
    a.refused(L.hfem_adam_multi_dev(a.di, T, 1, 1, 0, S, 1, K, a.st), M, b"bad sizes")
    a.refused(L.hfem_adam_multi_dev(a.di, T, -1, 1, 256, S, 1, K, a.st), M, b"bad sizes")
    a.refused(L.hfem_adam_multi_dev(a.di, T, 1, -1, 256, S, 1, K, a.st), M, b"bad sizes")
    a.refused(L.hfem_adam_multi_dev(a.di, None, 1, 1, 256, S, 1, K, a.st), M, b"null table")
    a.refused(L.hfem_adam_multi_dev(a.di, T, 1, 1, 256, S, 1, None, a.st), M, b"a device step counter needs a ticket counter")
    a.refused(L.hfem_adam_multi_dev(a.di, T, 1, 1, 256, None, 0, None, a.st), M, b"need a device step counter or a host step >= 1")
    assert L.hfem_adam_multi_dev(a.di, None, 0, 1, 256, None, 0, None, a.st) == 0                # an empty table, an empty grid: nothing to do
    assert L.hfem_adam_multi_dev(a.di, None, 1, 0, 256, None, 0, None, a.st) == 0
    a.refused(L.hfem_counter_add(a.di, None, 1, a.st), b"hfem_counter_add:", b"null pointer")
    a.refused(L.hfem_adam_prep(a.di, None, 0.9, 0.999, a.ptr(bc), a.st), b"hfem_adam_prep:", b"null pointer")
    a.refused(L.hfem_adam_prep(a.di, S, 0.9, 0.999, None, a.st), b"hfem_adam_prep:", b"null pointer")
    torch.cuda.synchronize()
    for k in "pmv":
        assert np.array_equal(b[k].get(k), d[k])
    assert np.array_equal(b["g"].get("g"), d["grads"][0])
    assert step.item() == 1 and not bc.any() and not ticket.any()


# ------------------------------------------------------------------------------------------------ E: special values
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_special_values(dtype):
    """E: entry by entry against adam_numpy: the same finiteness class and sign; zeros and non-finite values exactly, the others
    within the bound (fp32: the one-step allowance; where fp32 overflows, longdouble is no reference)."""
    a, T = Abi(), A.NP[dtype]
    allow = allowance(dtype, 1)
    for name, c in A.special_cases(dtype):
        want = A.adam_numpy(c["p"], c["g"], c["m"], c["v"], c["step"], **c["hyper"], dtype=T)
        b = {k: Buf(c[k], a.d, k) for k in "pgmv"}
        a.ok(a.L.hfem_adam_step(a.di, b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, 4, DT[dtype], *hyper_args(c["hyper"]), c["step"], a.st),
             "hfem_adam_step")
        torch.cuda.synchronize()
        for k, w in zip("pmv", want):
            got = b[k].get(f"E {name} {k}")
            assert np.array_equal(np.isnan(got), np.isnan(w)) and np.array_equal(np.isinf(got), np.isinf(w)), (name, k, got, w)
            assert np.array_equal(np.signbit(got), np.signbit(w)), (name, k, got, w)
            exact = ~np.isfinite(w) | (w == 0)
            assert np.array_equal(got[exact], w[exact]), (name, k, got, w)
            if name == "zero gradient, zero state" or (name in ("g*g overflows", "g*g underflows") and k == "p"):
                assert got.tobytes() == c[k].tobytes(), (name, k)
            err = A.rel_err(got[~exact], w[~exact])
            bound = A.ADAM_RTOL if dtype == F64 else allow[k]
            print(f"E {dtype} {name} {k}: err {err:.3e}, err / bound {err / bound:.3f}")
            assert err <= bound, (name, k, got, w)


def test_adam_prep_counts_and_bias_corrections():
    """E: three calls: the counter is 3 and bc = {1 - b1^3, sqrt(1 - b2^3)} within 4 ulp."""
    a = Abi()
    step = torch.zeros(1, dtype=torch.int64, device=a.d)
    bc = Buf(np.zeros(2), a.d, "p")
    for k in range(3):
        a.ok(a.L.hfem_adam_prep(a.di, a.ptr(step), 0.9, 0.999, bc.ptr, a.st), "hfem_adam_prep")
        torch.cuda.synchronize()
        assert step.item() == k + 1
        want = np.array([1.0 - 0.9 ** (k + 1), np.sqrt(1.0 - 0.999 ** (k + 1))])
        got = bc.get("bc")
        print(f"E adam_prep step {k + 1}: off by {np.abs(got - want) / np.spacing(want)} ulp")
    assert (np.abs(got - want) <= 4 * np.spacing(want)).all()


# ------------------------------------------------------------------------------------------------ F: through FusedAdam
def adam_pair(a, datas, dtype, capturable, hyper=A.HYPER, offset=0):
    """FusedAdam and torch.optim.Adam(foreach=False) on the GPU over the same values -> (fused params, torch params, both
    optimisers, the bases the fused parameters are views of)."""
    from hidenn_fem_amd.optim import FusedAdam
    bases = [Buf(d["p"], a.d, "p", offset) for d in datas]
    fused = [torch.nn.Parameter(b.view) for b in bases]
    plain = [torch.nn.Parameter(torch.from_numpy(d["p"].copy()).to(a.d)) for d in datas]
    kw = dict(lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"])
    return fused, plain, FusedAdam(fused, capturable=capturable, **kw), torch.optim.Adam(plain, foreach=False, **kw), bases


def pair_held(a, fused, plain, opt, ref, bases, dtype, steps, what):
    allow = allowance(dtype, steps, True)
    torch.cuda.synchronize()
    for i, (p, q, base) in enumerate(zip(fused, plain, bases)):
        base.get(f"{what} parameter {i}")
        for name, got, want in (("p", p, q), ("m", opt.state[p]["exp_avg"], ref.state[q]["exp_avg"]),
                                ("v", opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])):
            got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
            err = A.rel_err(got, want)
            bound = A.ADAM_RTOL if dtype == F64 else allow[name]
            print(f"{what} parameter {i} {name}: against torch.optim.Adam {err:.3e}, err / bound {err / bound:.3f}")
            assert np.isfinite(got).all() and err <= bound, (what, i, name)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_fused_adam_single_tensor_takes_the_host_step_launch(dtype):
    """F: one tensor, not capturable: ``hfem_adam_step``."""
    a, steps = Abi(), 6
    d = A.adam_data(1531, dtype, 61, steps, zero_state=True)
    fused, plain, opt, ref, bases = adam_pair(a, [d], dtype, False)
    for k in range(steps):
        fused[0].grad, plain[0].grad = (torch.from_numpy(d["grads"][k].copy()).to(a.d) for _ in range(2))
        opt.step()
        ref.step()
    assert opt.state[fused[0]]["step"] == steps
    pair_held(a, fused, plain, opt, ref, bases, dtype, steps, f"F single {dtype}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_fused_adam_follows_per_parameter_step_counts(dtype):
    """F: the second tensor has no gradient on step 3 of 6: the counts diverge, the per-tensor launches run and each follows
    its own count, as torch's do."""
    a, steps = Abi(), 6
    datas = [A.adam_data(n, dtype, 62 + n, steps, zero_state=True) for n in (1531, 1030)]
    fused, plain, opt, ref, bases = adam_pair(a, datas, dtype, False)
    for k in range(steps):
        for i, d in enumerate(datas):
            skip = i == 1 and k == 2
            fused[i].grad, plain[i].grad = (None if skip else torch.from_numpy(d["grads"][k].copy()).to(a.d) for _ in range(2))
        opt.step()
        ref.step()
    assert [opt.state[p]["step"] for p in fused] == [6, 5] and [int(ref.state[q]["step"]) for q in plain] == [6, 5]
    pair_held(a, fused, plain, opt, ref, bases, dtype, steps, f"F diverging counts {dtype}")


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_fused_adam_on_an_offset_view(dtype, capturable):
    """F: ``torch.nn.Parameter(base[1:])``: a contiguous parameter that does not start on a 16-byte boundary (moments and
    gradients do); the element in front of it stays as it was."""
    a, steps = Abi(), 6
    d = A.adam_data(1531, dtype, 64, steps, zero_state=True)
    fused, plain, opt, ref, bases = adam_pair(a, [d], dtype, capturable, offset=1)
    assert fused[0].data_ptr() % 16 != 0 and fused[0].is_contiguous()
    for k in range(steps):
        fused[0].grad, plain[0].grad = (torch.from_numpy(d["grads"][k].copy()).to(a.d) for _ in range(2))
        opt.step()
        ref.step()
    pair_held(a, fused, plain, opt, ref, bases, dtype, steps, f"F offset view {dtype} capturable={capturable}")
    if capturable:
        assert opt._step_dev.item() == steps and not opt._ticket.any()


def test_fused_adam_refuses_a_non_contiguous_parameter():
    from hidenn_fem_amd.optim import FusedAdam
    a = Abi()
    p = torch.nn.Parameter(torch.ones((8, 2), dtype=F64, device=a.d)[:, 0])
    p.grad = torch.ones(8, dtype=F64, device=a.d)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        FusedAdam([p]).step()
    torch.cuda.synchronize()
    assert (p == 1).all()
