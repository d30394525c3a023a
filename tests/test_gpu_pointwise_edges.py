"""The per-point (csrc/tri3_eval.hip), planless atomic (tri3_energy.hip, quad4.hip), post-processing (post.hip), row-assembly
and row-Adam (optim.hip) kernels at the launch forms and edges no other test reaches, against the CPU statements of
tests/pointwise_cases.py (``oracle.ref_chain`` + autograd, ``oracle.quad4``, ``oracle.closed_form``; the cases themselves are
pinned by tests/test_pointwise_cases_host.py):

  A  TRI3 per-point forward / backward through the C ABI, both gradient conventions: M = 1 .. 2048 * 256 + 1 (the second
     trip of the grid-stride loop), ids as arange / a multiset with repeats / 4096 points in one clockwise element, points on
     vertices, edge midpoints, the centroid and outside; NaN-poisoned forward outputs, prefilled (accumulated) gradients,
     every subset of {cu, cd, cg} as NULL; one near-degenerate element against the longdouble restatement
  B  EDGE2 per-point forward / backward the same way (edges in both directions, xi at 0, 1, inside, outside)
  C  the same kernels through ``PiecewiseLinearShapeNN2D(...)(x_eval, elem_id)`` and ``(..., edge=True)`` with ``.backward()``:
     repeated ids, expanded cotangents, tile-major rows, no boundary mask, an fp32 model, refused ``elem_id`` dtypes
  D  planless atomic energies: element ranges with ``e_begin > 0``, the loss-only instances, accumulation, the per-edge
     traction table, item counts past the grid cap
  E  von Mises (TRI3, QUAD4) and 1D slopes at ne = 1 .. 8192 * 256 + 1, ``grad_u`` given and NULL, dim_u = 1, 2, 3
  F  scatter / gather of rows, width 1, 2, 3, past the grid cap
  G  ``hfem_adam_step_rows_dev`` with ``hfem_counter_add`` against the fp64 formula
  H  empty and refused calls of every entry point above

Bounds are the project's own (tests/test_gpu_parity.py, tests/test_gpu_post.py; named in
tests/pointwise_cases.py).  The near-degenerate element alone has a derived one: 8 x the error the fp64 oracle itself shows
against the longdouble restatement (recorded in tests/test_pointwise_cases_host.py).  On an MI355X the kernels sit within
1e-2 of every bound of A, B, C and E, 0.13 of the gradient bound of D (QUAD4, 1 048 577 cells), 0.06 of G's; the fp32 model is
the fp64 one rounded, without a single differing ulp; on the near-degenerate element the kernel's error is 0.99 of the
oracle's own (the edge differences' roundings, shared by both, dominate).  The whole file takes 3 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pointwise_cases as K

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
GUARD = 64
CONV = {"reference": 0, "physical": 1}


def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


class Abi:
    def __init__(self):
        from hidenn_fem_amd import _lib
        self.lib, self.L, self.d = _lib, _lib.lib(), dev()
        self.di, self.st, self.ptr = _lib.dev_index(self.d), _lib.stream_ptr(self.d), _lib.ptr

    def ok(self, rc, what):
        self.lib.check(rc, what)

    def refused(self, rc, *needles):
        msg = self.L.hfem_last_error() or b""
        assert rc != 0 and all(n in msg for n in needles), (rc, msg, needles)


def dvec(a):
    a = [float(v) for v in np.asarray(a).reshape(-1)]
    return (C.c_double * len(a))(*a)


# ------------------------------------------------------------------------------------------------ buffers and comparisons
def guarded(shape, fill, d, dtype=F64):
    """A flat buffer of prod(shape) elements of ``fill`` (a number or a tensor) with GUARD NaNs behind them."""
    n = int(np.prod(shape))
    t = torch.full((n + GUARD,), NAN, dtype=dtype, device=d)
    t[:n] = fill if not torch.is_tensor(fill) else fill.reshape(-1).to(d)
    return t


def body(t, shape, what):
    """The payload of a guarded buffer, on the CPU; its guard must be intact."""
    n = int(np.prod(shape))
    assert torch.isnan(t[n:]).all(), f"{what}: wrote past its end"
    return t[:n].reshape(shape).cpu()


def prefill(shape, scale):
    """A nonzero pattern of the gradients' magnitude: what an accumulating kernel must add to."""
    n = int(np.prod(shape))
    return (scale * (0.5 + torch.frac(0.37 * torch.arange(1, n + 1, dtype=F64)))).reshape(shape)


def close(got, want, rtol, atol, what):
    got, want = got.detach().cpu().to(F64), torch.as_tensor(want, dtype=F64)
    got = got.reshape(want.shape)
    err, tol = (got - want).abs(), rtol * want.abs() + atol
    worst = (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: max err {err.max().item() if err.numel() else 0.0:.3e}, worst err/tol {worst:.3e}")
    assert torch.isfinite(got).all(), what
    assert (err <= tol).all(), f"{what}: worst err/tol {worst:.3e}"


def close_grad(got, want, what):
    """tests/test_gpu_parity.py assert_grad_close: max-abs error against GRAD_RTOL x max|g| (an all-zero gradient: exactly)."""
    want = torch.as_tensor(want, dtype=F64)
    close(got, want, 0.0, K.GRAD_RTOL * want.abs().max().item(), what)


def close_loss(got, want, what):
    close(torch.as_tensor(got, dtype=F64), torch.as_tensor(want, dtype=F64), K.LOSS_RTOL, 0.0, what)


def ulp32(t):
    a = t.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(F64)


def close32(got, want64, what):
    """An fp32 result equal, within one fp32 rounding, to the fp64 result rounded."""
    assert got.dtype == F32, what
    got, r = got.detach().cpu(), want64.detach().cpu().to(F32)
    err = (got.to(F64) - r.to(F64)).abs().reshape(-1)
    print(f"{what}: worst err / ulp {(err / ulp32(r).reshape(-1)).max().item():.3f}")
    assert (err <= ulp32(r).reshape(-1)).all(), what


# ------------------------------------------------------------------------------------------------ A, B: running the C ABI
def to_dev(c, keys):
    d = dev()
    out = {}
    for k in keys:
        t = c[k]
        out[k] = (t.to(torch.int32) if k in ("conn", "edges") else t).contiguous().to(d)
    return out


def run_tri3_fwd(a, g, m, conv, entry="hfem_tri3_eval_fwd_conv"):
    """-> (u_h [m,2], detJ [m], grad_u [m,2,2]) on the CPU; the outputs start NaN-poisoned and guarded."""
    u_h, detJ, grad_u = guarded((m, 2), NAN, a.d), guarded((m,), NAN, a.d), guarded((m, 2, 2), NAN, a.d)
    args = [a.di, a.ptr(g["X"]), a.ptr(g["U"]), a.ptr(g["conn"]), a.ptr(g["x_eval"]), a.ptr(g["elem_id"]), m, a.ptr(u_h), a.ptr(detJ),
            a.ptr(grad_u)] + ([conv] if entry.endswith("_conv") else []) + [a.st]
    a.ok(getattr(a.L, entry)(*args), entry)
    torch.cuda.synchronize()
    return body(u_h, (m, 2), "u_h"), body(detJ, (m,), "detJ"), body(grad_u, (m, 2, 2), "grad_u")


def run_tri3_bwd(a, g, m, conv, cots, pre_x, pre_u, zeros_for_missing=False, entry="hfem_tri3_eval_bwd_conv"):
    """-> (gX, gU) on the CPU, accumulated onto pre_x / pre_u.  A cotangent not in ``cots`` is NULL, or a zero tensor."""
    gX, gU = guarded(pre_x.shape, pre_x, a.d), guarded(pre_u.shape, pre_u, a.d)
    cot = {k: g[k] if k in cots else (torch.zeros_like(g[k]) if zeros_for_missing else None) for k in ("cu", "cd", "cg")}
    args = [a.di, a.ptr(g["X"]), a.ptr(g["U"]), a.ptr(g["conn"]), a.ptr(g["x_eval"]), a.ptr(g["elem_id"]), m, a.ptr(cot["cu"]),
            a.ptr(cot["cd"]), a.ptr(cot["cg"]), a.ptr(gX), a.ptr(gU)] + ([conv] if entry.endswith("_conv") else []) + [a.st]
    a.ok(getattr(a.L, entry)(*args), entry)
    torch.cuda.synchronize()
    return body(gX, pre_x.shape, "gX"), body(gU, pre_u.shape, "gU")


TRI3_KEYS = ("X", "U", "conn", "x_eval", "elem_id", "cu", "cd", "cg")
TRI3_CASES = [("multiset", m) for m in K.POINT_M] + [("arange", None), ("one", K.ONE_ELEMENT_M), ("special", None)]


@pytest.mark.parametrize("convention", ["reference", "physical"])
@pytest.mark.parametrize("ids,m", TRI3_CASES)
def test_tri3_eval_sizes_ids_and_points(ids, m, convention):
    """A: every size and id pattern, forward into NaN-poisoned outputs, backward onto a nonzero pattern."""
    a, c = Abi(), K.tri3_case(ids, m)
    want = K.tri3_expected_cached(ids, m, convention)
    m, g, what = c["elem_id"].shape[0], to_dev(c, TRI3_KEYS), f"A {ids} {m} {convention}"
    if ids != "one" and m > 1:
        assert (want["detJ"] < 0).any() and (want["detJ"] > 0).any()                  # both orientations were sampled
    u_h, detJ, grad_u = run_tri3_fwd(a, g, m, CONV[convention])
    close(u_h, want["u_h"], K.U_RTOL, 0.0, what + " u_h")
    close(detJ, want["detJ"], K.U_RTOL, 0.0, what + " detJ")
    close(grad_u, want["grad_u"], K.GRADU_RTOL, K.GRADU_ATOL, what + " grad_u")
    pre_x = prefill(c["X"].shape, want["gX"].abs().max().item())
    pre_u = prefill(c["U"].shape, want["gU"].abs().max().item())
    gX, gU = run_tri3_bwd(a, g, m, CONV[convention], ("cu", "cd", "cg"), pre_x, pre_u)
    close_grad(gX - pre_x, want["gX"], what + " gX")
    close_grad(gU - pre_u, want["gU"], what + " gU")
    if convention == "reference" and m == 257:                  # the entries without a convention argument are the reference one
        for x, y in zip(run_tri3_fwd(a, g, m, 0), run_tri3_fwd(a, g, m, None, entry="hfem_tri3_eval_fwd")):
            assert torch.equal(x, y)
        gX2, gU2 = run_tri3_bwd(a, g, m, None, ("cu", "cd", "cg"), pre_x, pre_u, entry="hfem_tri3_eval_bwd")
        close_grad(gX2 - pre_x, want["gX"], what + " gX (hfem_tri3_eval_bwd)")
        close_grad(gU2 - pre_u, want["gU"], what + " gU (hfem_tri3_eval_bwd)")


@pytest.mark.parametrize("convention", ["reference", "physical"])
def test_tri3_eval_cotangent_subsets(convention):
    """A: every subset of {cu, cd, cg} given, the others NULL: the oracle's gradient of those terms alone, the same as the
    full call with the others zeroed, and nothing at all (bit for bit) when all three are NULL."""
    a, c = Abi(), K.tri3_case("multiset", 257)
    g, conv = to_dev(c, TRI3_KEYS), CONV[convention]
    full = K.tri3_expected_cached("multiset", 257, convention)
    pre_x, pre_u = prefill(c["X"].shape, full["gX"].abs().max().item()), prefill(c["U"].shape, full["gU"].abs().max().item())
    for cots in K.COT_SUBSETS:
        what = f"A subset {'+'.join(cots) or 'none'} {convention}"
        want = K.tri3_expected(c, convention, cots)
        gX, gU = run_tri3_bwd(a, g, 257, conv, cots, pre_x, pre_u)
        if not cots:
            assert torch.equal(gX, pre_x) and torch.equal(gU, pre_u), what + ": an all-NULL call changed the gradients"
            continue
        close_grad(gX - pre_x, want["gX"], what + " gX")
        close_grad(gU - pre_u, want["gU"], what + " gU")
        zX, zU = run_tri3_bwd(a, g, 257, conv, cots, pre_x, pre_u, zeros_for_missing=True)
        close(gX, zX, 0.0, K.GRAD_RTOL * want["gX"].abs().max().item(), what + " gX against zeroed cotangents")
        close(gU, zU, 0.0, K.GRAD_RTOL * want["gU"].abs().max().item(), what + " gU against zeroed cotangents")


@pytest.mark.parametrize("convention", ["reference", "physical"])
def test_tri3_eval_near_degenerate_element(convention):
    """A: aspect 1e6.  detJ, grad_u and the gradients against the longdouble restatement, allowed DEGENERATE_FACTOR = 8 x the
    error the fp64 oracle shows against it (tests/test_pointwise_cases_host.py records it: 1.0e-12 relative for detJ, grad_u
    and gU, 2.0e-12 for gX); u_h keeps rtol 1e-13."""
    a, c = Abi(), K.degenerate_case()
    m, g = c["elem_id"].shape[0], to_dev(c, TRI3_KEYS)
    ld, allow = K.tri3_closed_form_ld(c, convention), K.DEGENERATE_REF_ERR[convention]
    u_h, detJ, grad_u = run_tri3_fwd(a, g, m, CONV[convention])
    zx, zu = torch.zeros_like(c["X"]), torch.zeros_like(c["U"])
    gX, gU = run_tri3_bwd(a, g, m, CONV[convention], ("cu", "cd", "cg"), zx, zu)
    close(u_h, torch.from_numpy(ld["u_h"].astype(np.float64)), K.U_RTOL, 0.0, f"A degenerate {convention} u_h")
    for k, got in (("detJ", detJ), ("grad_u", grad_u), ("gX", gX), ("gU", gU)):
        err = K.max_err_ld(got, ld[k])
        print(f"A degenerate {convention} {k}: max err {err:.4e}, oracle's own {allow[k]:.4e}, ratio {err / allow[k]:.3f}")
        assert torch.isfinite(got).all()
    for k, got in (("detJ", detJ), ("grad_u", grad_u), ("gX", gX), ("gU", gU)):
        assert K.max_err_ld(got, ld[k]) <= K.DEGENERATE_FACTOR * allow[k], (convention, k)


EDGE2_KEYS = ("X", "U", "edges", "xi", "edge_id", "cu", "cd")
EDGE2_CASES = [("multiset", m) for m in K.POINT_M] + [("arange", None), ("one", K.ONE_ELEMENT_M), ("special", None)]


def run_edge2_fwd(a, g, m):
    u_h, ds = guarded((m, 2), NAN, a.d), guarded((m,), NAN, a.d)
    a.ok(a.L.hfem_edge2_eval_fwd(a.di, a.ptr(g["X"]), a.ptr(g["U"]), a.ptr(g["edges"]), a.ptr(g["xi"]), a.ptr(g["edge_id"]), m,
                                 a.ptr(u_h), a.ptr(ds), a.st), "hfem_edge2_eval_fwd")
    torch.cuda.synchronize()
    return body(u_h, (m, 2), "u_h"), body(ds, (m,), "ds")


def run_edge2_bwd(a, g, m, cots, pre_x, pre_u, with_u=True):
    gX, gU = guarded(pre_x.shape, pre_x, a.d), guarded(pre_u.shape, pre_u, a.d)
    a.ok(a.L.hfem_edge2_eval_bwd(a.di, a.ptr(g["X"]), a.ptr(g["U"]) if with_u else None, a.ptr(g["edges"]), a.ptr(g["xi"]),
                                 a.ptr(g["edge_id"]), m, a.ptr(g["cu"]) if "cu" in cots else None,
                                 a.ptr(g["cd"]) if "cd" in cots else None, a.ptr(gX), a.ptr(gU), a.st), "hfem_edge2_eval_bwd")
    torch.cuda.synchronize()
    return body(gX, pre_x.shape, "gX"), body(gU, pre_u.shape, "gU")


@pytest.mark.parametrize("ids,m", EDGE2_CASES)
def test_edge2_eval_sizes_ids_and_points(ids, m):
    """B: forward and backward of the edge branch at every size and id pattern; the ds gradient against autograd AND the
    closed form +-c (Xj - Xi) / |Xj - Xi|."""
    a, c = Abi(), K.edge2_case(ids, m)
    want = K.edge2_expected_cached(ids, m)
    m, g, what = c["edge_id"].shape[0], to_dev(c, EDGE2_KEYS), f"B {ids} {m}"
    u_h, ds = run_edge2_fwd(a, g, m)
    close(u_h, want["u_h"], K.U_RTOL, 0.0, what + " u_h")
    close(ds, want["ds"], K.U_RTOL, 0.0, what + " ds")
    pre_x, pre_u = prefill(c["X"].shape, want["gX"].abs().max().item()), prefill(c["U"].shape, want["gU"].abs().max().item())
    gX, gU = run_edge2_bwd(a, g, m, ("cu", "cd"), pre_x, pre_u)
    close_grad(gX - pre_x, want["gX"], what + " gX")
    close_grad(gX - pre_x, K.edge2_ds_gradient(c), what + " gX (closed form)")
    close_grad(gU - pre_u, want["gU"], what + " gU")


def test_edge2_eval_cotangent_subsets():
    """B: cu alone, cds alone, both, neither (a no-op, bit for bit); U is not read by the backward and may be NULL."""
    a, c = Abi(), K.edge2_case("multiset", 257)
    g, full = to_dev(c, EDGE2_KEYS), K.edge2_expected_cached("multiset", 257)
    pre_x, pre_u = prefill(c["X"].shape, full["gX"].abs().max().item()), prefill(c["U"].shape, full["gU"].abs().max().item())
    for cots in ((), ("cu",), ("cd",), ("cu", "cd")):
        want = K.edge2_expected(c, cots)
        gX, gU = run_edge2_bwd(a, g, 257, cots, pre_x, pre_u, with_u=bool(cots) and cots != ("cd",))
        if "cd" not in cots:
            assert torch.equal(gX, pre_x), f"B subset {cots}: gX changed without a ds cotangent"
        else:
            close_grad(gX - pre_x, want["gX"], f"B subset {cots} gX")
            close_grad(gX - pre_x, K.edge2_ds_gradient(c), f"B subset {cots} gX (closed form)")
        if "cu" not in cots:
            assert torch.equal(gU, pre_u), f"B subset {cots}: gU changed without a u_h cotangent"
        else:
            close_grad(gU - pre_u, want["gU"], f"B subset {cots} gU")


# ------------------------------------------------------------------------------------------------ C: through the model
def build_model(c, variant, X, u_free, u_fixed):
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    m = PiecewiseLinearShapeNN2D(X, c["conn"], boundary_mask=None if variant == "no_boundary" else c["boundary_mask"],
                                 dirichlet_mask=c["dirichlet_mask"], u_fixed=u_fixed, neumann_edges=c["edges"],
                                 reorder="tile" if variant == "tile" else "auto").to(dev())
    assert m.row_order == ("tile" if variant == "tile" else "as given") and m.dtype == X.dtype
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(u_free, "u").to(dev()))
    return m


def run_model(m, c):
    """Both branches with the weighted scalar losses of ``pointwise_cases.model_expected`` -> the same dict, gradients in the
    caller's row order."""
    d = dev()
    out = {}
    u_h, detJ, grad_u = m(c["x_eval"].to(d), c["elem_id"].to(d))
    (c["w_u"] * u_h.sum() + c["w_d"] * detJ.sum() + c["w_g"] * grad_u.sum()).backward()
    grads = lambda: (m.to_caller_order(m.node_coords_free.grad, "x").detach().clone(), m.to_caller_order(m.u_free.grad, "u").detach().clone())
    out["tri"] = (u_h.detach(), detJ.detach(), grad_u.detach()) + grads()
    m.zero_grad(set_to_none=True)
    u_h, ds = m(c["xi"].to(d), c["edge_id"].to(d), edge=True)
    (c["w_u"] * u_h.sum() + c["w_s"] * ds.sum()).backward()
    out["edge"] = (u_h.detach(), ds.detach()) + grads()
    m.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("variant", ["plain", "tile", "no_boundary"])
def test_model_forward_backward_with_repeated_ids(variant):
    """C: ``model(x_eval, elem_id)`` and ``model(x, edge_id, edge=True)`` with ``.backward()`` of a ``.sum()`` loss (cotangents
    arrive expanded), ids repeating about twenty times; parameter gradients against the oracle chain -- rows as given, tile-major
    rows given back through ``to_caller_order``, and a model without a boundary mask."""
    c = K.model_case()
    want = K.model_expected(c, with_boundary=variant != "no_boundary")
    m = build_model(c, variant, c["X"], c["u_free"], torch.tensor(K.U_FIXED, dtype=F64))
    got = run_model(m, c)
    what = f"C {variant}"
    close(got["tri"][0], want["tri"][0], K.U_RTOL, 0.0, what + " u_h")
    close(got["tri"][1], want["tri"][1], K.U_RTOL, 0.0, what + " detJ")
    close(got["tri"][2], want["tri"][2], K.GRADU_RTOL, K.GRADU_ATOL, what + " grad_u")
    close_grad(got["tri"][3], want["tri"][3], what + " node_coords_free.grad")
    close_grad(got["tri"][4], want["tri"][4], what + " u_free.grad")
    close(got["edge"][0], want["edge"][0], K.U_RTOL, 0.0, what + " edge u_h")
    close(got["edge"][1], want["edge"][1], K.U_RTOL, 0.0, what + " ds")
    close_grad(got["edge"][2], want["edge"][2], what + " edge node_coords_free.grad")
    close_grad(got["edge"][3], want["edge"][3], what + " edge u_free.grad")
    assert want["edge"][2].abs().max() > 0 and want["tri"][3].abs().max() > 0


def test_model_fp32_is_the_fp64_model_rounded_once():
    """C: an fp32 model gives float32 outputs and gradients equal, within one fp32 rounding, to those of the fp64 model on the
    same (widened) parameters; the fp64 model on them is itself held to the oracle."""
    c = K.model_case()
    X32, u32, f32 = c["X"].to(F32), c["u_free"].to(F32), torch.tensor(K.U_FIXED, dtype=F32)
    m32 = build_model(c, "plain", X32, u32, f32)
    m64 = build_model(c, "plain", X32.to(F64), u32.to(F64), f32.to(F64))
    got, twin = run_model(m32, c), run_model(m64, c)
    for branch in ("tri", "edge"):
        for k, (g32, g64) in enumerate(zip(got[branch], twin[branch])):
            close32(g32, g64, f"C fp32 {branch}[{k}]")
    # the twin itself against the oracle on the widened parameters (the Dirichlet value is the fp32 one, widened)
    X64 = X32.to(F64)
    want = K.model_expected(dict(c, X=X64), coords_free=X64[~c["boundary_mask"]], u_free=u32.to(F64), u_fixed=f32.to(F64).item())
    close(twin["tri"][0], want["tri"][0], K.U_RTOL, 0.0, "C fp32 twin u_h")
    close(twin["tri"][2], want["tri"][2], K.GRADU_RTOL, K.GRADU_ATOL, "C fp32 twin grad_u")
    close_grad(twin["tri"][3], want["tri"][3], "C fp32 twin node_coords_free.grad")
    close_grad(twin["tri"][4], want["tri"][4], "C fp32 twin u_free.grad")
    close_grad(twin["edge"][2], want["edge"][2], "C fp32 twin edge node_coords_free.grad")
    close_grad(twin["edge"][3], want["edge"][3], "C fp32 twin edge u_free.grad")


def run_quad_model(c, X, u_free, u_fixed, x_eval, elem_id):
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    d = dev()
    m = PiecewiseLinearShapeNN2D(X, K.quad_mesh()["conn"], boundary_mask=c["boundary_mask"], dirichlet_mask=c["dirichlet_mask"],
                                 u_fixed=u_fixed).to(d)
    with torch.no_grad():
        m.u_free.copy_(u_free.to(d))
    got = m(x_eval.to(d), elem_id.to(d))
    (c["w_u"] * got[0].sum() + c["w_d"] * got[1].sum() + c["w_g"] * got[2].sum()).backward()
    assert all(t.dtype == X.dtype for t in got) and m.u_free.grad.dtype == X.dtype
    return [t.detach() for t in got] + [m.node_coords_free.grad, m.u_free.grad]


def test_quad4_model_backward_with_expanded_cotangents():
    """C, the QUAD4 per-point wrapper (its backward materialises three cotangent copies as the edge branch does two): a
    ``.sum()`` loss with repeated ids against ``oracle.quad4`` + autograd, and the fp32 model against the fp64 one on the
    widened parameters, within one fp32 rounding."""
    c = K.model_case()
    x_eval, elem_id, u_h, detJ, grad_u, gx, gu = K.quad_model_expected(c)
    got = run_quad_model(c, c["X"], c["u_free"], torch.tensor(K.U_FIXED, dtype=F64), x_eval, elem_id)
    close(got[0], u_h, K.U_RTOL, 0.0, "C quad4 u_h")
    close(got[1], detJ, K.U_RTOL, 0.0, "C quad4 detJ")
    close(got[2], grad_u, K.GRADU_RTOL, K.GRADU_ATOL, "C quad4 grad_u")
    close_grad(got[3], gx, "C quad4 node_coords_free.grad")
    close_grad(got[4], gu, "C quad4 u_free.grad")
    X32, u32, f32 = c["X"].to(F32), c["u_free"].to(F32), torch.tensor(K.U_FIXED, dtype=F32)
    got32 = run_quad_model(c, X32, u32, f32, x_eval, elem_id)
    twin = run_quad_model(c, X32.to(F64), u32.to(F64), f32.to(F64), x_eval, elem_id)
    for k, (g32, g64) in enumerate(zip(got32, twin)):
        close32(g32, g64, f"C quad4 fp32 [{k}]")


def test_model_refuses_ids_of_another_dtype_or_on_the_cpu():
    c = K.model_case()
    m = build_model(c, "plain", c["X"], c["u_free"], torch.tensor(K.U_FIXED, dtype=F64))
    d = dev()
    x, xi = c["x_eval"].to(d), c["xi"].to(d)
    for bad in (torch.int32, torch.int16, torch.float64):
        with pytest.raises(RuntimeError, match="must be torch.int64"):
            m(x, c["elem_id"].to(bad).to(d))
        with pytest.raises(RuntimeError, match="must be torch.int64"):
            m(xi, c["edge_id"].to(bad).to(d), edge=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, c["elem_id"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(xi, c["edge_id"], edge=True)


# ------------------------------------------------------------------------------------------------ D: planless atomic energies
def energy_inputs(kind):
    mesh = K.quad_mesh() if kind == "quad4" else K.tri_mesh()
    X = mesh["X"]
    U = K.u_positive(X.shape[0]) if kind == "edge2" else K.u_strain(X)
    return X.to(dev()), U.to(dev())


def run_energy(a, kind, X, U, items, lo, hi, loss, gX, gU, T=None, Tconst=None):
    """One call of the planless entry of ``kind`` on items [lo, hi) (EDGE2: the first ``hi`` edges) -> rc."""
    nn = X.shape[0]
    if kind == "tri3":
        return a.L.hfem_tri3_energy_atomic(a.di, a.ptr(X), a.ptr(U), a.ptr(items), lo, hi, nn, dvec(K.energy_mat()), K.ENERGY_W,
                                           dvec(K.energy_bk()), a.ptr(loss), a.ptr(gX), a.ptr(gU), a.st)
    if kind == "quad4":
        return a.L.hfem_quad4_energy_atomic(a.di, a.ptr(X), a.ptr(U), a.ptr(items), lo, hi, nn, dvec(K.energy_mat()), a.ptr(loss),
                                            a.ptr(gX), a.ptr(gU), a.st)
    return a.L.hfem_edge2_energy_atomic(a.di, a.ptr(X), a.ptr(U), a.ptr(items), hi, a.ptr(T), None if Tconst is None else dvec(Tconst),
                                        a.ptr(loss), a.ptr(gX), a.ptr(gU), a.st)


def energy_expected(kind, n):
    if kind == "tri3":
        items, e, gX, gU = K.tri3_energy_expected(n)
        return items, None, e, gX, gU
    if kind == "quad4":
        items, e, gX, gU = K.quad4_energy_expected(n)
        return items, None, e, gX, gU
    return K.edge2_energy_expected(n)


@pytest.mark.parametrize("kind,n", [("tri3", n) for n in K.ENERGY_N] + [("quad4", n) for n in K.QUAD4_N] + [("edge2", n) for n in K.ENERGY_N])
def test_atomic_energy_sizes_accumulate_and_loss_only(kind, n):
    """D: one item, a second block of one item, and one item past the grid cap (rows of the tiny mesh repeated) against the
    plain-C closed forms on the same rows; loss and gradients accumulate onto prefilled values; the loss-only instance
    (gX = gU = NULL) gives the same loss.  EDGE2 reads the per-edge table (distinct rows, Tconst NULL)."""
    a = Abi()
    items, T, e, gX_ref, gU_ref = energy_expected(kind, n)
    X, U = energy_inputs(kind)
    it, Td = items.to(torch.int32).to(a.d), None if T is None else T.to(a.d)
    pre_l = 0.37 * abs(e)
    pre_x, pre_u = prefill(X.shape, np.abs(gX_ref).max()), prefill(U.shape, np.abs(gU_ref).max())
    loss, gX, gU = guarded((1,), pre_l, a.d), guarded(X.shape, pre_x, a.d), guarded(U.shape, pre_u, a.d)
    a.ok(run_energy(a, kind, X, U, it, 0, n, loss, gX, gU, T=Td), kind)
    only = guarded((1,), pre_l, a.d)
    a.ok(run_energy(a, kind, X, U, it, 0, n, only, None, None, T=Td), kind + " loss-only")
    torch.cuda.synchronize()
    what = f"D {kind} n={n}"
    close_loss(body(loss, (1,), "loss")[0] - pre_l, e, what + " loss")
    close_loss(body(only, (1,), "loss")[0] - pre_l, e, what + " loss-only loss")
    close_loss(body(only, (1,), "loss")[0], body(loss, (1,), "loss")[0], what + " loss-only against the gradient call")
    close_grad(body(gX, X.shape, "gX") - pre_x, gX_ref, what + " gX")
    close_grad(body(gU, U.shape, "gU") - pre_u, gU_ref, what + " gU")


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_atomic_energy_ranges_add_up(kind):
    """D: [0,7) [7,7) [7,29) [29,ne) -- uneven, one empty, three with e_begin > 0 or e_end < ne -- add to the whole call in loss
    and gradients (and to the closed form), with and without gradients; no range touches another's elements (the first
    range alone is the closed form of its rows)."""
    from oracle import closed_form as CF
    a = Abi()
    mesh = K.quad_mesh() if kind == "quad4" else K.tri_mesh()
    ne = mesh["conn"].shape[0]
    items, _, e, gX_ref, gU_ref = energy_expected(kind, ne)
    X, U = energy_inputs(kind)
    it = items.to(torch.int32).to(a.d)
    cuts = (0,) + tuple(min(c, ne) for c in K.ENERGY_RANGES) + (ne,)
    loss, only = guarded((1,), 0.0, a.d), guarded((1,), 0.0, a.d)
    gX, gU = guarded(X.shape, 0.0, a.d), guarded(U.shape, 0.0, a.d)
    parts = []
    for lo, hi in zip(cuts, cuts[1:]):
        one = guarded((1,), 0.0, a.d)
        a.ok(run_energy(a, kind, X, U, it, lo, hi, one, None, None), f"{kind} [{lo},{hi}) loss-only")
        a.ok(run_energy(a, kind, X, U, it, lo, hi, loss, gX, gU), f"{kind} [{lo},{hi})")
        a.ok(run_energy(a, kind, X, U, it, lo, hi, only, None, None), f"{kind} [{lo},{hi}) loss-only")
        parts.append((lo, hi, one))
    whole_l, whole_x, whole_u = guarded((1,), 0.0, a.d), guarded(X.shape, 0.0, a.d), guarded(U.shape, 0.0, a.d)
    a.ok(run_energy(a, kind, X, U, it, 0, ne, whole_l, whole_x, whole_u), kind)
    torch.cuda.synchronize()
    what = f"D {kind} ranges"
    Xn, Un = X.cpu().numpy(), U.cpu().numpy()
    for lo, hi, one in parts:                                   # each range is the closed form of exactly its rows
        rows = items[lo:hi].numpy()
        if kind == "tri3":
            want = CF.tri3_energy(Xn, Un, rows, K.energy_mat(), K.ENERGY_W, K.energy_bk(), grads=False)[0] if hi > lo else 0.0
        else:
            want = CF.quad4_energy(Xn, Un, rows, K.energy_mat(), grads=False)[0] if hi > lo else 0.0
        got = body(one, (1,), "loss")[0]
        if hi > lo:
            close_loss(got, want, f"{what} [{lo},{hi}) loss")
        else:
            assert got.item() == 0.0
    close_loss(body(loss, (1,), "loss")[0], e, what + " summed loss")
    close_loss(body(only, (1,), "loss")[0], e, what + " summed loss-only loss")
    close_loss(body(loss, (1,), "loss")[0], body(whole_l, (1,), "loss")[0], what + " summed loss against the whole call")
    close_grad(body(gX, X.shape, "gX"), gX_ref, what + " gX")
    close_grad(body(gU, U.shape, "gU"), gU_ref, what + " gU")
    close_grad(body(gX, X.shape, "gX"), body(whole_x, X.shape, "gX"), what + " gX against the whole call")
    close_grad(body(gU, U.shape, "gU"), body(whole_u, U.shape, "gU"), what + " gU against the whole call")


def test_edge2_atomic_table_wins_over_the_constant():
    """D: T and Tconst both given behave as T alone; Tconst alone is another number (the table is what was read)."""
    a = Abi()
    edges, T, e, gX_ref, gU_ref = K.edge2_energy_expected(257)
    X, U = energy_inputs("edge2")
    it, Td = edges.to(torch.int32).to(a.d), T.to(a.d)
    res = {}
    for tag, (t, tc) in dict(both=(Td, [9e9, -7e9, 5e9, 1e9]), const=(None, T[0].numpy())).items():
        loss, gX, gU = guarded((1,), 0.0, a.d), guarded(X.shape, 0.0, a.d), guarded(U.shape, 0.0, a.d)
        a.ok(run_energy(a, "edge2", X, U, it, 0, 257, loss, gX, gU, T=t, Tconst=tc), "edge2 " + tag)
        torch.cuda.synchronize()
        res[tag] = (body(loss, (1,), "loss")[0], body(gX, X.shape, "gX"), body(gU, U.shape, "gU"))
    close_loss(res["both"][0], e, "D edge2 T and Tconst loss")
    close_grad(res["both"][1], gX_ref, "D edge2 T and Tconst gX")
    close_grad(res["both"][2], gU_ref, "D edge2 T and Tconst gU")
    assert abs(res["const"][0].item() - e) > 1e-3 * abs(e)


def test_atomic_energy_refusals_leave_the_outputs_untouched():
    """D: gX without gU (and the reverse), neither T nor Tconst, e_end < e_begin, a negative edge count: nonzero, with their
    messages, nothing written."""
    a = Abi()
    tri, quad = K.tri_mesh(), K.quad_mesh()
    X, U = energy_inputs("tri3")
    ct, cq, ed = (t.to(torch.int32).to(a.d) for t in (tri["conn"], quad["conn"], tri["edges"]))
    Td = K.edge_tractions(ed.shape[0]).to(a.d)
    pre_x, pre_u = prefill(X.shape, 1.0), prefill(U.shape, 2.0)
    loss, gX, gU = guarded((1,), 0.125, a.d), guarded(X.shape, pre_x, a.d), guarded(U.shape, pre_u, a.d)
    for kind, items in (("tri3", ct), ("quad4", cq)):
        ne = items.shape[0]
        a.refused(run_energy(a, kind, X, U, items, 0, ne, loss, gX, None), b"gX and gU must both be given or both NULL")
        a.refused(run_energy(a, kind, X, U, items, 0, ne, loss, None, gU), b"gX and gU must both be given or both NULL")
        a.refused(run_energy(a, kind, X, U, items, 5, 4, loss, gX, gU), b"bad element range")
        a.refused(run_energy(a, kind, X, U, items, -1, 4, loss, gX, gU), b"bad element range")
    ned = ed.shape[0]
    a.refused(run_energy(a, "edge2", X, U, ed, 0, ned, loss, gX, None, T=Td), b"gX and gU must both be given or both NULL")
    a.refused(run_energy(a, "edge2", X, U, ed, 0, ned, loss, None, gU, T=Td), b"gX and gU must both be given or both NULL")
    a.refused(run_energy(a, "edge2", X, U, ed, 0, ned, loss, gX, gU), b"need a per-edge traction table or a constant one")
    a.refused(run_energy(a, "edge2", X, U, ed, 0, -1, loss, gX, gU, T=Td), b"negative edge count")
    torch.cuda.synchronize()
    assert body(loss, (1,), "loss")[0].item() == 0.125
    assert torch.equal(body(gX, X.shape, "gX"), pre_x) and torch.equal(body(gU, U.shape, "gU"), pre_u)


# ------------------------------------------------------------------------------------------------ E: post-processing
@pytest.mark.parametrize("n", K.POST_N)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_von_mises_sizes_and_optional_grad_u(kind, n):
    """E: ne = 1, one block, one element more, and one past the grid cap (rows repeated), on a mesh with clockwise elements,
    E = 3, nu = 0.45; grad_u given and NULL: the same vm bit for bit."""
    a = Abi()
    X, U, conn, g_ref, vm_ref = K.von_mises_base(kind)
    pick = torch.arange(n) % conn.shape[0]
    it = conn[pick].to(torch.int32).contiguous().to(a.d)
    Xd, Ud = X.to(a.d), U.to(a.d)
    entry = getattr(a.L, f"hfem_{kind}_von_mises")
    vm, gu, vm2 = guarded((n,), NAN, a.d), guarded((n, 2, 2), NAN, a.d), guarded((n,), NAN, a.d)
    a.ok(entry(a.di, a.ptr(Xd), a.ptr(Ud), a.ptr(it), n, K.POST_E, K.POST_NU, a.ptr(vm), a.ptr(gu), a.st), kind)
    a.ok(entry(a.di, a.ptr(Xd), a.ptr(Ud), a.ptr(it), n, K.POST_E, K.POST_NU, a.ptr(vm2), None, a.st), kind)
    torch.cuda.synchronize()
    vm, gu, vm2 = body(vm, (n,), "vm"), body(gu, (n, 2, 2), "grad_u"), body(vm2, (n,), "vm")
    close(gu, torch.from_numpy(g_ref)[pick], K.POST_GRADU_RTOL, K.POST_GRADU_ATOL, f"E {kind} n={n} grad_u")
    close(vm, torch.from_numpy(vm_ref)[pick], K.VM_RTOL, 0.0, f"E {kind} n={n} vm")
    assert torch.equal(vm, vm2), "vm depends on whether grad_u was asked for"


@pytest.mark.parametrize("dim_u", [1, 2, 3])
def test_line2_slopes_sizes_and_components(dim_u):
    """E: n_nodes = 0, 1 (nothing written, rc 0), 2, 257 and past the grid cap, on a non-uniform grid."""
    a = Abi()
    for n in K.slope_nodes(dim_u):
        grid, u, want = K.slopes_case(n, dim_u)
        n_out = max(n - 1, 0) * dim_u
        gd, ud = grid.to(a.d), u.contiguous().to(a.d)
        out = guarded((max(n_out, 8),), NAN, a.d)
        a.ok(a.L.hfem_line2_slopes(a.di, a.ptr(gd), a.ptr(ud), n, dim_u, a.ptr(out), a.st), "hfem_line2_slopes")
        torch.cuda.synchronize()
        if n < 2:
            assert torch.isnan(out).all(), f"n_nodes = {n} wrote something"
            continue
        assert torch.isnan(out[n_out:]).all(), "wrote past its end"
        close(out[:n_out].cpu(), want, K.SLOPE_RTOL, K.SLOPE_ATOL, f"E slopes dim_u={dim_u} n={n}")
        if n <= 257:
            close(out[:n_out].cpu(), K.slopes_by_autograd(grid, u), K.SLOPE_RTOL, K.SLOPE_ATOL, f"E slopes dim_u={dim_u} n={n} (autograd)")


# ------------------------------------------------------------------------------------------------ F: row assembly
@pytest.mark.parametrize("width", K.ROW_WIDTHS)
def test_scatter_gather_rows(width):
    """F: a random permutation as the index: scatter is the statement dst[idx[r]] = src[r] bit for bit, gather after scatter
    the identity; a free set and a fixed set cover a poisoned destination exactly once; rows = 0 writes nothing."""
    a = Abi()
    for rows in K.row_counts(width):
        src, idx = K.rows_case(rows, width)
        sd, idd = src.to(a.d), idx.to(a.d)
        dst, back = guarded((max(rows, 4), width), NAN, a.d), guarded((max(rows, 4), width), NAN, a.d)
        a.ok(a.L.hfem_scatter_rows(a.di, a.ptr(sd), a.ptr(idd), rows, width, a.ptr(dst), a.st), "hfem_scatter_rows")
        a.ok(a.L.hfem_gather_rows(a.di, a.ptr(dst), a.ptr(idd), rows, width, a.ptr(back), a.st), "hfem_gather_rows")
        torch.cuda.synchronize()
        if rows == 0:
            assert torch.isnan(dst).all() and torch.isnan(back).all()
            continue
        want = torch.empty_like(src)
        want[idx.long()] = src
        assert torch.equal(body(dst, (max(rows, 4), width), "dst")[:rows], want), f"F scatter width={width} rows={rows}"
        assert torch.equal(body(back, (max(rows, 4), width), "back")[:rows], src), f"F gather after scatter width={width} rows={rows}"
        assert rows >= 4 or torch.isnan(dst[rows * width:]).all()
        # free + fixed: two disjoint index sets, together every row once
        k = rows // 3
        dst2 = guarded((rows, width), NAN, a.d)
        free_idx, fixed_idx = idd[:k].contiguous(), idd[k:].contiguous()
        a.ok(a.L.hfem_scatter_rows(a.di, a.ptr(sd[:k].contiguous()), a.ptr(free_idx), k, width, a.ptr(dst2), a.st), "scatter free")
        torch.cuda.synchronize()
        assert int(torch.isnan(dst2[:rows * width].reshape(rows, width)[:, 0]).sum()) == rows - k          # the free set alone: k rows
        a.ok(a.L.hfem_scatter_rows(a.di, a.ptr(sd[k:].contiguous()), a.ptr(fixed_idx), rows - k, width, a.ptr(dst2), a.st), "scatter fixed")
        torch.cuda.synchronize()
        assert torch.equal(body(dst2, (rows, width), "dst2"), want), f"F free + fixed width={width} rows={rows}"
    for bad in (0, -1):
        a.refused(a.L.hfem_scatter_rows(a.di, a.ptr(sd), a.ptr(idd), 1, bad, a.ptr(dst), a.st), b"hfem_scatter_rows", b"bad shape")
        a.refused(a.L.hfem_gather_rows(a.di, a.ptr(sd), a.ptr(idd), 1, bad, a.ptr(dst), a.st), b"hfem_gather_rows", b"bad shape")
    a.refused(a.L.hfem_scatter_rows(a.di, a.ptr(sd), a.ptr(idd), -1, width, a.ptr(dst), a.st), b"bad shape")


# ------------------------------------------------------------------------------------------------ G: row Adam
def test_adam_step_rows_dev_matches_the_formula():
    """G: five steps on 137 listed rows of a [300][2] tensor, the step read from a device counter that hfem_counter_add
    advances: listed rows within 1e-14 relative of torch.optim.Adam's formula in fp64, the other rows of p, m, v untouched
    bit for bit; n_rows = 0 is a no-op with NULL pointers."""
    a, c = Abi(), K.adam_case()
    p, m, v, rows = c["p"].to(a.d), c["m"].to(a.d), c["v"].to(a.d), c["rows"].to(a.d)
    step = torch.zeros(1, dtype=torch.int64, device=a.d)
    pn, mn, vn = c["p"].numpy().copy(), c["m"].numpy().copy(), c["v"].numpy().copy()
    h = K.ADAM_HYPER
    assert a.L.hfem_adam_step_rows_dev(a.di, None, None, None, None, None, 0, h["lr"], h["beta1"], h["beta2"], h["eps"], None, a.st) == 0
    for k, g in enumerate(c["grads"]):
        gd = g.to(a.d)
        a.ok(a.L.hfem_counter_add(a.di, a.ptr(step), 1, a.st), "hfem_counter_add")
        a.ok(a.L.hfem_adam_step_rows_dev(a.di, a.ptr(p), a.ptr(gd), a.ptr(m), a.ptr(v), a.ptr(rows), K.ADAM_LISTED, h["lr"], h["beta1"],
                                         h["beta2"], h["eps"], a.ptr(step), a.st), "hfem_adam_step_rows_dev")
        torch.cuda.synchronize()
        assert step.item() == k + 1
        pn, mn, vn = K.adam_rows_numpy(pn, g.numpy(), mn, vn, c["rows"].numpy(), k + 1, **h)
    listed = torch.zeros(K.ADAM_N, dtype=torch.bool)
    listed[c["rows"].long()] = True
    for name, got, want, init in (("p", p, pn, c["p"]), ("m", m, mn, c["m"]), ("v", v, vn, c["v"])):
        got = got.cpu()
        assert torch.equal(got[~listed], init[~listed]), f"G {name}: an unlisted row changed"
        close(got[listed], torch.from_numpy(want)[listed], K.ADAM_RTOL, 0.0, f"G {name}")
        assert (got[listed] != init[listed]).all()


# ------------------------------------------------------------------------------------------------ H: empty and refused calls
def entry_points(a):
    """name -> (argument list of a small valid call, positions of its required pointers, its output tensors)."""
    tri, quad = K.tri_mesh(), K.quad_mesh()
    d, P = a.d, a.ptr
    X, U = tri["X"].to(d), K.u_strain(tri["X"]).to(d)
    ct, cq, ed = (t.to(torch.int32).to(d) for t in (tri["conn"], quad["conn"], tri["edges"]))
    m = 4
    xe, xi = K.random_points(m, 1).to(d), K.random_points(m, 2)[:, 0].contiguous().to(d)
    eid = torch.arange(m, device=d)
    cot = {k: t.to(d) for k, t in K._cotangents(m, 3).items()}
    nn, ne, nq, ned = X.shape[0], ct.shape[0], cq.shape[0], ed.shape[0]
    o = lambda *shape: torch.full(shape, NAN, dtype=F64, device=d)
    u_h, detJ, gu, ds, gX, gU, loss, vm, vgu = o(m, 2), o(m), o(m, 2, 2), o(m), o(nn, 2), o(nn, 2), o(1), o(ne), o(ne, 2, 2)
    sl, rows_out = o(nn - 1, 2), o(nn, 2)
    idx = torch.randperm(nn, generator=torch.Generator().manual_seed(4)).to(torch.int32).to(d)
    grid = torch.cumsum(torch.ones(nn, dtype=F64), 0).to(d)
    T = K.edge_tractions(ned).to(d)
    mat, bk, tc = dvec(K.energy_mat()), dvec(K.energy_bk()), dvec([1.0, 2.0, 3.0, 4.0])
    am, av, step = o(nn, 2), o(nn, 2), torch.ones(1, dtype=torch.int64, device=d)
    outs = [u_h, detJ, gu, ds, gX, gU, loss, vm, vgu, sl, rows_out, am, av]
    h = K.ADAM_HYPER
    table = {
        "hfem_tri3_eval_fwd_conv": ([a.di, P(X), P(U), P(ct), P(xe), P(eid), m, P(u_h), P(detJ), P(gu), 0, a.st], (1, 2, 3, 4, 5, 7, 8, 9)),
        "hfem_tri3_eval_bwd_conv": ([a.di, P(X), P(U), P(ct), P(xe), P(eid), m, P(cot["cu"]), P(cot["cd"]), P(cot["cg"]), P(gX), P(gU), 0,
                                     a.st], (1, 2, 3, 4, 5, 10, 11)),
        "hfem_edge2_eval_fwd": ([a.di, P(X), P(U), P(ed), P(xi), P(eid), m, P(u_h), P(ds), a.st], (1, 2, 3, 4, 5, 7, 8)),
        "hfem_edge2_eval_bwd": ([a.di, P(X), P(U), P(ed), P(xi), P(eid), m, P(cot["cu"]), P(cot["cd"]), P(gX), P(gU), a.st], (1, 3, 4, 5, 9, 10)),
        "hfem_tri3_energy_atomic": ([a.di, P(X), P(U), P(ct), 0, ne, nn, mat, K.ENERGY_W, bk, P(loss), P(gX), P(gU), a.st], (1, 2, 3, 7, 10)),
        "hfem_quad4_energy_atomic": ([a.di, P(X), P(U), P(cq), 0, nq, nn, mat, P(loss), P(gX), P(gU), a.st], (1, 2, 3, 7, 8)),
        "hfem_edge2_energy_atomic": ([a.di, P(X), P(U), P(ed), ned, P(T), tc, P(loss), P(gX), P(gU), a.st], (1, 2, 3, 7)),
        "hfem_tri3_von_mises": ([a.di, P(X), P(U), P(ct), ne, 3.0, 0.45, P(vm), P(vgu), a.st], (1, 2, 3, 7)),
        "hfem_quad4_von_mises": ([a.di, P(X), P(U), P(cq), nq, 3.0, 0.45, P(vm), P(vgu), a.st], (1, 2, 3, 7)),
        "hfem_line2_slopes": ([a.di, P(grid), P(U), nn, 2, P(sl), a.st], (1, 2, 5)),
        "hfem_scatter_rows": ([a.di, P(U), P(idx), nn, 2, P(rows_out), a.st], (1, 2, 5)),
        "hfem_gather_rows": ([a.di, P(U), P(idx), nn, 2, P(rows_out), a.st], (1, 2, 5)),
        "hfem_adam_step_rows_dev": ([a.di, P(rows_out), P(U), P(am), P(av), P(idx), nn, h["lr"], h["beta1"], h["beta2"], h["eps"], P(step),
                                     a.st], (1, 2, 3, 4, 5, 11)),
    }
    keep = (X, U, ct, cq, ed, xe, xi, eid, cot, idx, grid, T, step, mat, bk, tc)
    return table, outs, keep


COUNT_AT = {"hfem_tri3_eval_fwd_conv": 6, "hfem_tri3_eval_bwd_conv": 6, "hfem_edge2_eval_fwd": 6, "hfem_edge2_eval_bwd": 6,
            "hfem_edge2_energy_atomic": 4, "hfem_tri3_von_mises": 4, "hfem_quad4_von_mises": 4, "hfem_line2_slopes": 3,
            "hfem_scatter_rows": 3, "hfem_gather_rows": 3, "hfem_adam_step_rows_dev": 6}


# pointer arguments that may be NULL in a non-empty call (the cotangents, U of the edge backward, gX / gU, Bk, T / Tconst, grad_u)
OPTIONAL_POINTERS = {"hfem_tri3_eval_bwd_conv": (7, 8, 9), "hfem_edge2_eval_bwd": (2, 7, 8), "hfem_tri3_energy_atomic": (9, 11, 12),
                     "hfem_quad4_energy_atomic": (9, 10), "hfem_edge2_energy_atomic": (5, 6, 8, 9), "hfem_tri3_von_mises": (8,),
                     "hfem_quad4_von_mises": (8,)}


def test_every_required_pointer_is_checked_and_empty_calls_need_none():
    """H: each required pointer NULL in turn: a nonzero code and a message that names the entry point and says "null pointer";
    a count of zero returns 0 with EVERY pointer NULL (the planless energies: an empty range, also one that starts past 0);
    an unknown convention and negative counts are refused.  No output is written by any of these calls."""
    a = Abi()
    table, outs, keep = entry_points(a)
    for name, (args, required) in table.items():
        fn = getattr(a.L, name)
        for pos in required:
            bad = list(args)
            bad[pos] = None
            a.refused(fn(*bad), name.encode(), b"null pointer")
        empty = [None if i in required or i in OPTIONAL_POINTERS.get(name, ()) else v for i, v in enumerate(args)]
        if name in COUNT_AT:
            for count in (0,):
                e = list(empty)
                e[COUNT_AT[name]] = count
                assert fn(*e) == 0, (name, a.L.hfem_last_error())
            e[COUNT_AT[name]] = -1
            a.refused(fn(*e), name.encode())
        else:                                                   # hfem_tri3_energy_atomic, hfem_quad4_energy_atomic: [e_begin, e_end)
            for lo in (0, 5):
                e = list(empty)
                e[4], e[5] = lo, lo
                assert fn(*e) == 0, (name, a.L.hfem_last_error())
    for name in ("hfem_tri3_eval_fwd_conv", "hfem_tri3_eval_bwd_conv"):
        for conv in (2, -1):
            bad = list(table[name][0])
            bad[-2] = conv
            a.refused(getattr(a.L, name)(*bad), name.encode(), b"unknown gradient convention")
    a.refused(a.L.hfem_line2_slopes(a.di, None, None, 0, 0, None, a.st), b"bad sizes")
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs)
    del keep
