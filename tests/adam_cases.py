"""Inputs, sizes and CPU statements for the launch-form edges of the Adam kernels (csrc/optim.hip), shared by
tests/test_adam_cases_host.py and tests/test_gpu_adam_edges.py (a plain helper module, not a conftest; nothing of the GPU
library is imported).

References.  ``adam_numpy`` restates one ``torch.optim.Adam`` step (no weight decay, no amsgrad) operation for operation in
``np.float64`` or, as ``adam_one<float>`` states it, in ``np.float32``: every scalar is computed in double and cast to float,
the square root is taken in double and rounded to float.  ``adam_longdouble`` is the same formula in ``np.longdouble`` on the
same (rounded) arrays with the hyper-parameters as the doubles they are.

Data.  ``adam_data(n, dtype, seed)`` is ``pointwise_cases.adam_case`` as a function: |p| in [0.5, 1.5), every gradient keeps
its entry's sign, m and v start with that sign and size (or at zero, as ``torch.optim.Adam`` starts), the total movement stays
below 0.05.  No step cancels, so "relative, per entry" is a fair demand on p, m and v.

Bounds.  fp64: ``ADAM_RTOL`` = 1e-14 per entry against ``adam_numpy`` (the project's own bound).  fp32: against
``adam_longdouble``, ``FP32_FACTOR`` = 4 times the largest per-entry error that ``adam_numpy`` in fp32 itself shows against
``adam_longdouble`` on ``ALLOW_N`` = 200 000 entries of the same data, for the same number of steps and the same
hyper-parameters (``fp32_allowance``): the kernel's own roundings plus the reference's, each of that size, with a factor 2 for
the kernel's contraction choices (it is built with -ffp-contract=on).  Nothing of it comes from a kernel's output.
"""
import functools

import numpy as np
import torch

from pointwise_cases import ADAM_HYPER, ADAM_RTOL, adam_rows_numpy      # noqa: F401  (re-exported)

F32, F64 = torch.float32, torch.float64
LD = np.longdouble
NP = {F64: np.float64, F32: np.float32}
FP32_FACTOR = 4
ALLOW_N = 200_000
HYPER = dict(ADAM_HYPER)                                # lr 1e-2, betas (0.9, 0.999), eps 1e-8
HYPER_B = dict(lr=3e-3, beta1=0.0, beta2=0.5, eps=1e-8)  # the betas=(0.0, 0.5) group

# ------------------------------------------------------------------------------------------------ sizes (csrc/optim.hip)
BLOCK = 256
GRID_CAP = 2048                                         # hfem_adam_step, hfem_adam_step_dev: if (grid > 2048) grid = 2048
VEC = {F64: 2, F32: 4}                                  # elements of one 16-byte vector
CAP = {dt: GRID_CAP * BLOCK * VEC[dt] for dt in VEC}     # the largest n the vector loop covers in one trip
ONE_TRIP_MORE = {dt: CAP[dt] + BLOCK * VEC[dt] + VEC[dt] - 1 for dt in VEC}   # + 256 vectors (block 0's second trip) + a full tail
LENGTHS = {F64: (1, 2, 3, 511, 512, 513, CAP[F64], ONE_TRIP_MORE[F64]),
           F32: (1, 3, 4, 5, 6, 7, 1023, 1024, 1025, CAP[F32], ONE_TRIP_MORE[F32])}
OFFSET_N = {F64: 513, F32: 1025}
STEPS, BIG_STEPS = 3, 2                                 # the four lengths from CAP on run BIG_STEPS


def steps_of(n, dtype):
    return BIG_STEPS if n >= CAP[dtype] else STEPS


def step_grid(n, dtype):
    """Blocks of hfem_adam_step / hfem_adam_step_dev."""
    return min(max((n // VEC[dtype] + BLOCK - 1) // BLOCK, 1), GRID_CAP)


def vector_trips(n, dtype, aligned=True):
    """Trips of block 0's thread 0 through the vector loop of adam_body (unaligned views: through the scalar loop)."""
    stride = step_grid(n, dtype) * BLOCK
    return -(-(n // VEC[dtype] if aligned else n) // stride)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the formula
def _scalars(step, lr, beta1, beta2, eps, T):
    """(w1, b2, w2, step_size, sqrt_bc2, eps) as the kernels form them: in double, then cast to T."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return T(1.0 - beta1), T(beta2), T(1.0 - beta2), T(lr / bc1), T(np.sqrt(bc2)), T(eps)


def adam_numpy(p, g, m, v, step, lr, beta1, beta2, eps, dtype=np.float64):
    """One step of torch.optim.Adam on whole arrays -> (p, m, v), in torch's association:
    m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, 1 - b2); p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)).
    ``dtype`` np.float32: adam_one<float> -- scalars cast to float first, the square root in double and rounded."""
    T = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a, dtype=T) for a in (p, g, m, v))
    w1, b2, w2, step_size, sqrt_bc2, eps = _scalars(step, lr, beta1, beta2, eps, T)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        m = m + w1 * (g - m)
        v = v * b2 + w2 * (g * g)
        denom = np.sqrt(v.astype(np.float64)).astype(T) / sqrt_bc2 + eps
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == T
    return p, m, v


def adam_longdouble(p, g, m, v, step, lr, beta1, beta2, eps):
    """The same formula in np.longdouble; arrays are taken as they are (fp32 / fp64 inputs widen exactly, a longdouble state
    of an earlier step is kept), the hyper-parameters are the doubles the caller passes."""
    p, g, m, v = (np.asarray(a).astype(LD) for a in (p, g, m, v))
    lr, beta1, beta2, eps = LD(lr), LD(beta1), LD(beta2), LD(eps)
    bc1, bc2 = 1 - beta1 ** LD(step), 1 - beta2 ** LD(step)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        m = m + (1 - beta1) * (g - m)
        v = v * beta2 + (1 - beta2) * (g * g)
        p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v


def run_steps(fn, d, steps, first_step=1, **kw):
    """``fn`` (adam_numpy / adam_longdouble) over d["grads"][:steps] from d's p, m, v -> list of (p, m, v) after each step."""
    p, m, v = d["p"], d["m"], d["v"]
    out = []
    for k in range(steps):
        p, m, v = fn(p, d["grads"][k], m, v, first_step + k, **kw)
        out.append((p, m, v))
    return out


def rel_err(got, want_ld):
    """max |got - want| / |want| per entry, the difference taken in longdouble (empty: 0)."""
    got, want_ld = np.asarray(got).astype(LD).reshape(-1), np.asarray(want_ld).astype(LD).reshape(-1)
    return float((np.abs(got - want_ld) / np.abs(want_ld)).max()) if got.size else 0.0


# ------------------------------------------------------------------------------------------------ data without cancellation
MAX_STEPS = 6


def adam_data(n, dtype, seed, steps=STEPS, zero_state=False):
    """-> dict(p, m, v: np arrays [n] of ``dtype``, grads: ``steps`` arrays).  Built in fp64 from a seeded generator, then
    rounded to ``dtype``; ``zero_state``: m = v = 0 (a fresh torch.optim.Adam)."""
    assert steps <= MAX_STEPS
    g = _gen(seed)
    sign = lambda: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).to(F64)
    p = sign() * (0.5 + torch.rand(n, generator=g, dtype=F64))
    g_base = sign() * (0.2 + torch.rand(n, generator=g, dtype=F64))
    m, v = 0.2 * g_base, 0.5 * g_base * g_base
    if zero_state:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    grads = [g_base * (1.0 + 0.3 * np.cos(1.7 * k)) * (0.8 + 0.4 * torch.rand(n, generator=g, dtype=F64)) for k in range(steps)]
    T = NP[dtype]
    return dict(p=p.numpy().astype(T), m=m.numpy().astype(T), v=v.numpy().astype(T), grads=[x.numpy().astype(T) for x in grads])


def _hyper_key(h):
    return (float(h["lr"]), float(h["beta1"]), float(h["beta2"]), float(h["eps"]))


@functools.lru_cache(maxsize=None)
def _reference(n, dtype, seed, steps, zero_state, first_step, hkey):
    h = dict(zip(("lr", "beta1", "beta2", "eps"), hkey))
    d = adam_data(n, dtype, seed, steps, zero_state)
    ref = run_steps(functools.partial(adam_numpy, dtype=NP[dtype]), d, steps, first_step, **h)
    ld = run_steps(adam_longdouble, d, steps, first_step, **h) if dtype == F32 else None
    for a in list(d.values())[:3] + d["grads"] + [x for r in ref for x in r]:
        a.setflags(write=False)                          # shared among tests: left unchanged
    if n >= CAP[dtype]:                                  # the big cases are compared after their last step only
        ref = [None] * (steps - 1) + ref[-1:]
        ld = ld and [None] * (steps - 1) + ld[-1:]
    return d, ref, ld


def reference(n, dtype, seed, steps=STEPS, zero_state=False, first_step=1, hyper=HYPER):
    """-> (data, [adam_numpy (p, m, v) after each step], [adam_longdouble ... ] or None for fp64); computed once."""
    return _reference(n, dtype, seed, steps, zero_state, first_step, _hyper_key(hyper))


@functools.lru_cache(maxsize=None)
def _fp32_allowance(steps, zero_state, hkey):
    _, ref, ld = _reference(ALLOW_N, F32, 1000 + steps, steps, zero_state, 1, hkey)
    return {name: FP32_FACTOR * max(rel_err(ref[k][i], ld[k][i]) for k in range(steps)) for i, name in enumerate("pmv")}


def fp32_allowance(steps=STEPS, zero_state=False, hyper=HYPER):
    """-> dict(p, m, v): FP32_FACTOR x the largest per-entry relative error of adam_numpy fp32 against adam_longdouble over
    ``steps`` steps (the worst of them) of ALLOW_N entries."""
    return _fp32_allowance(steps, bool(zero_state), _hyper_key(hyper))


def fp32_reference_errors(steps, zero_state=False, hyper=HYPER):
    return {k: a / FP32_FACTOR for k, a in fp32_allowance(steps, zero_state, hyper).items()}


# ------------------------------------------------------------------------------------------------ B: two tensors, listed rows
ROWS_X, ROWS_U = 600, 500
ROW_SPLITS = ((100, 300), (256, 1), (255, 2), (0, 137), (137, 0))
LR_X, LR_U = 1e-2, 3e-3


def rows2_case(n_x, n_u, dtype, seed=7):
    """-> dict(x, u: adam_data of ROWS_X * 2 / ROWS_U * 2 entries ([rows][2] flat), rows_x, rows_u: int32 subsets in random
    order)."""
    g = _gen(seed + 13 * n_x + n_u)
    rows_x = torch.randperm(ROWS_X, generator=g)[:n_x].to(torch.int32)
    rows_u = torch.randperm(ROWS_U, generator=g)[:n_u].to(torch.int32)
    return dict(x=adam_data(ROWS_X * 2, dtype, seed + 1), u=adam_data(ROWS_U * 2, dtype, seed + 2), rows_x=rows_x, rows_u=rows_u)


def rows_expected(d, rows, steps, lr, dtype, ld=False):
    """The references on the listed rows alone (the formula is per entry): -> list over steps of (p, m, v) [len(rows), 2]."""
    r = np.asarray(rows, dtype=np.int64)
    sub = dict(p=d["p"].reshape(-1, 2)[r], m=d["m"].reshape(-1, 2)[r], v=d["v"].reshape(-1, 2)[r],
               grads=[x.reshape(-1, 2)[r] for x in d["grads"]])
    h = dict(HYPER, lr=lr)
    fn = adam_longdouble if ld else functools.partial(adam_numpy, dtype=NP[dtype])
    return run_steps(fn, sub, steps, **h)


# ------------------------------------------------------------------------------------------------ C: multi-tensor tables
CHUNKS = (1, 255, 256, 257, 300, 512)
TICKET_BLOCKS = (1, 2, 31, 32, 33, 63, 64, 65, 100)
TICKET_CLASSES = 32                                     # kAdamTicketClasses
MANY_BLOCKS = 6000                                      # more blocks than an MI355X holds at once (256 CUs x 8)


def seven_tensors(chunk):
    """The table of C: (n, dtype, hyper, offset elements, blocks or None = what the tensor needs)."""
    return [
        (1500 * 2 + 1, F64, dict(HYPER, lr=1.0e-2), 0, None),       # in-chunk trips, a partial last block, a tail
        (3, F32, dict(HYPER, lr=9e-3), 0, None),                    # no vector: one block, tail only
        (0, F64, dict(HYPER, lr=8e-3), 0, None),                    # one block, no work
        (1025, F32, dict(HYPER, lr=7e-3), 0, None),
        (700, F64, dict(HYPER, lr=6e-3), 1, 2),                     # unaligned: block 0 does everything, block 1 nothing
        (514, F64, dict(HYPER_B), 0, None),                         # betas (0.0, 0.5)
        (2 * chunk, F64, dict(HYPER, lr=5e-3), 0, None),            # exactly one chunk
    ]


def blocks_needed(n, dtype, chunk, aligned=True):
    nv = n // VEC[dtype] if aligned else 0
    return max(1, -(-nv // chunk))


def table_layout(tensors, chunk):
    """-> (block_begin of every tensor, total blocks)."""
    begin, blk = [], 0
    for n, dtype, _, off, blocks in tensors:
        begin.append(blk)
        blk += blocks if blocks is not None else blocks_needed(n, dtype, chunk, off == 0)
    return begin, blk


def table_cover(tensors, chunk, n_blocks):
    """What adam_multi_dev_kernel's blocks 0 .. n_blocks - 1 touch, restated: -> one int array [n] of visit counts per tensor.
    Block B works on the last tensor t with block_begin[t] <= B, on the vectors [b chunk, (b + 1) chunk) below nv; block b = 0
    of a tensor takes the elements from nv * N on (everything, when the tensor is not 16-byte aligned)."""
    begin, _ = table_layout(tensors, chunk)
    counts = [np.zeros(n, dtype=np.int64) for n, *_ in tensors]
    for B in range(n_blocks):
        t = max(i for i, b0 in enumerate(begin) if b0 <= B)
        n, dtype, _, off, _ = tensors[t]
        N = VEC[dtype]
        nv = n // N if off == 0 else 0
        b = B - begin[t]
        counts[t][min(b * chunk, nv) * N:min((b + 1) * chunk, nv) * N] += 1
        if b == 0:
            counts[t][nv * N:] += 1
    return counts


def fused_table_layout(numels, dtypes):
    """``FusedAdam._table`` restated: -> (chunk, block_begin per tensor, blocks)."""
    total = sum(-(-n // VEC[dt]) for n, dt in zip(numels, dtypes))
    chunk = -(-max(256, -(-total // 2048)) // 256) * 256
    begin, blk = [], 0
    for n, dt in zip(numels, dtypes):
        begin.append(blk)
        blk += max(1, -(-(n // VEC[dt]) // chunk))
    return chunk, begin, blk


# ------------------------------------------------------------------------------------------------ E: special values
def special_cases(dtype):
    """-> list of (name, dict(p, g, m, v: arrays [4], step, hyper)).  Expected values are adam_numpy's."""
    T = NP[dtype]
    big = 1e200 if dtype == F64 else 1e30
    a = lambda *x: np.array(x, dtype=T)
    p0 = a(1.0, -0.75, 0.5, -1.25)
    out = [
        ("zero gradient, zero state", dict(p=p0, g=a(0, 0, 0, 0), m=a(0, 0, 0, 0), v=a(0, 0, 0, 0), step=1, hyper=HYPER)),
        ("g*g overflows", dict(p=p0, g=a(big, -big, big, -big), m=a(0.1, -0.1, 0, 0), v=a(0.5, 0.5, 0, 0), step=2, hyper=HYPER)),
        ("step 10^6", dict(p=p0, g=a(0.3, -0.4, 0.5, -0.6), m=a(0.2, -0.3, 0.4, -0.5), v=a(0.1, 0.2, 0.3, 0.4), step=10 ** 6, hyper=HYPER)),
        ("beta1 = 0", dict(p=p0, g=a(0.3, -0.4, 0.5, -0.6), m=a(0.2, -0.3, 0.4, -0.5), v=a(0.1, 0.2, 0.3, 0.4), step=3,
                           hyper=dict(HYPER, beta1=0.0))),
        ("eps = 0", dict(p=p0, g=a(0.3, -0.4, 0.5, -0.6), m=a(0.2, -0.3, 0.4, -0.5), v=a(0.1, 0.2, 0.3, 0.4), step=3,
                         hyper=dict(HYPER, eps=0.0))),
    ]
    if dtype == F32:
        out.append(("g*g underflows", dict(p=p0, g=a(1e-30, -1e-30, 1e-30, -1e-30), m=a(1e-30, -1e-30, 2e-30, -2e-30),
                                           v=a(0, 0, 0, 0), step=1, hyper=HYPER)))
    return out
