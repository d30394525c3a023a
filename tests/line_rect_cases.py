"""Inputs and CPU statement for the edge cases of the 1D / structured-grid kernels (csrc/line_rect.hip), shared by
tests/test_line_rect_cases_host.py and tests/test_gpu_line_rect_edges.py (a plain helper module, not a conftest).

Every input is built deterministically on the CPU in fp64 (seeded ``torch.Generator``).  The expected results are stated
with ``oracle.ref_chain`` (``grid_param``, ``masked_grid``, ``line2_forward``, ``mse_loss``, ``rectq4_forward``) and torch
autograd; what is missing there is added here: ``dudx`` as a differentiable expression, and the bar energy on given
``(xq, wq, bq)`` (``ops.BarEnergyFn`` takes them detached).  fp32 expectations are this fp64 statement of the fp32-rounded
inputs (``round32``).

The functions that state a result take the forward they differentiate as an argument (``forward=R.line2_forward`` ...), so
that the host test can run the same statement over a copy of the forward with one rule changed.
"""
import math

import torch

from oracle import ref_chain as R

F32, F64 = torch.float32, torch.float64
EPS_H = 1e-10                              # reference src/models.py:43


# ------------------------------------------------------------------------------------------------ tolerances of the GPU test
# (stated here so that the host test's mutation checks measure against the very numbers the GPU test asserts)
GRID_RTOL, GRID_ATOL = 1e-12, 1e-13        # fp64 grids (tests/test_gpu_post.py)
GP_RTOL, GP_ATOL_REL = 1e-9, 1e-12         # increments' gradient: rtol, atol = GP_ATOL_REL * max|g| (tests/test_gpu_post.py)
LOSS_RTOL, GRAD_RTOL = 1e-12, 1e-10        # losses; accumulated gradients relative to max|g| (tests/test_gpu_parity.py)
POINT_RTOL = 1e-12                         # per-point outputs, relative to the summed magnitudes of their terms
CLAMP_RTOL = 1e-11                         # case F gradients, relative to sum_q |contribution of point q|
SMALL_N = 11                               # up to here the grid is held to GRID_ATOL alone (see grid_tol)


def grid_tol(ref, n):
    """Elementwise tolerance of an fp64 grid.  For n <= SMALL_N the relative part is dropped: with at most 11 positive
    terms per running sum and a softplus good to about 2 ulp, x0 + L cum/S is off by at most ~14 u on cum and on S, i.e.
    3 * 3.6e-15 + ulp(5) = 1.2e-14 absolute for L = 3 -- GRID_ATOL = 1e-13 is eight times that worst case.  This is
    TIGHTER than the project's tolerance, and it has to be: torch's softplus takes ``x > 20``, and ``x >= 20`` moves the
    n = 11 grid by 3.6e-11, only 10 x (GRID_RTOL |g| + GRID_ATOL) but 350 x GRID_ATOL."""
    return GRID_ATOL + (GRID_RTOL * ref.abs() if n > SMALL_N else 0.0)


def gp_tol(ref):
    return GP_RTOL * ref.abs() + GP_ATOL_REL * ref.abs().max()


def round32(t):
    """The fp64 tensor a float-row kernel sees: rounded to fp32 and widened again."""
    return t.to(F32).to(F64)


def _leaf(t, on):
    return t.detach().clone().requires_grad_(bool(on))


# ------------------------------------------------------------------------------------------------ A, B, C: grid parametrisation
INC_CYCLE = [-30.0, -14.5, -13.0, 0.0, 3.0, 19.5, 20.0, 20.5, 25.0, -2.0, 0.7]
X0, XN = 2.0, 5.0
ONE_BLOCK_N = (1, 2, 11, 1023, 1024, 1025, 2047, 2048)    # through ops.GridParamFn (one workgroup up to 2048)
ONE_BLOCK_ABI_N = 4097                                     # chunk = 5, idle threads beyond tid 819: C ABI only
WS_SMALL_N = (2, 11, 1023, 1024, 1025)                     # _ws forms below the Python threshold: C ABI only (11: v == 20.0
                                                           # is only told from ``>= 20`` at a small n, see grid_tol)
WS_LONG_N = 1024 * 1024 + 1                                # 1025 blocks: gp_block_offsets_kernel's chunk becomes 2
SOFTPLUS_KNIFE = math.log(math.expm1(1e-6))                # softplus(v) == 1e-6: a last-bit difference flips the clamp


def grid_param_case(n, use_mask):
    """Case A/B inputs: increments cycling through INC_CYCLE, cotangent cos(0.37 k); the mask has both ends plus about n/8
    interior entries, ``initial`` is a linspace."""
    p = torch.tensor([INC_CYCLE[k % len(INC_CYCLE)] for k in range(n)], dtype=F64)
    cot = torch.cos(0.37 * torch.arange(n + 1, dtype=F64))
    mask = initial = None
    if use_mask:
        g = torch.Generator().manual_seed(1000 + n)
        mask = torch.zeros(n + 1, dtype=torch.bool)
        mask[0] = mask[-1] = True
        if n > 2:
            mask[torch.randint(1, n, (max(1, n // 8),), generator=g)] = True
        initial = torch.linspace(X0, XN, n + 1, dtype=F64)
    return dict(p=p, cot=cot, mask=mask, initial=initial, x0=X0, xN=XN)


def grid_param_long_case():
    """Case C inputs: n = 1024 * 1024 + 1, increments 0.3 randn with -30 on every 97th row and 25 on every 211th row from
    row 5, both ends masked."""
    n = WS_LONG_N
    g = torch.Generator().manual_seed(n)
    p = 0.3 * torch.randn(n, generator=g, dtype=F64)
    p[::97] = -30.0
    p[5::211] = 25.0
    mask = torch.zeros(n + 1, dtype=torch.bool)
    mask[0] = mask[-1] = True
    cot = torch.cos(0.37 * torch.arange(n + 1, dtype=F64))
    return dict(p=p, cot=cot, mask=mask, initial=torch.linspace(X0, XN, n + 1, dtype=F64), x0=X0, xN=XN)


def grid_param_expected(case, grid_fn=R.grid_param):
    """-> (grid [n+1], gp [n]) of reference src/models.py:45-56, 146-168 for one case dict (fp64 statement of its inputs)."""
    p = _leaf(case["p"], True)
    grid = grid_fn(p, torch.tensor([case["x0"]], dtype=F64), torch.tensor([case["xN"]], dtype=F64))
    if case["mask"] is not None:
        grid = R.masked_grid(grid, case["mask"], case["initial"])
    (grid * case["cot"]).sum().backward()
    return grid.detach(), p.grad


def grid_param_blocked(case, block=1024):
    """The same grid with the running sums taken in another legitimate order: cumsum inside blocks of ``block`` increments
    plus an exclusive cumsum of the block totals (what a multi-workgroup scan does).  Only used to MEASURE how far the fp64
    statement moves between two summation orders."""
    inc = torch.clamp(torch.nn.functional.softplus(case["p"]), min=1e-6)
    n = inc.shape[0]
    pad = (-n) % block
    blocks = torch.cat([inc, inc.new_zeros(pad)]).reshape(-1, block)
    local = torch.cumsum(blocks, dim=1)
    tot = local[:, -1]
    off = torch.cumsum(tot, dim=0) - tot
    cum = (local + off[:, None]).reshape(-1)[:n]
    grid = torch.cat([torch.tensor([case["x0"]], dtype=F64), case["x0"] + (case["xN"] - case["x0"]) * cum / cum[-1]])
    return grid if case["mask"] is None else R.masked_grid(grid, case["mask"], case["initial"])


def grid_param_buffer_sizes(n, ws_elems):
    """Element counts of the C-ABI buffers of the grid parametrisation for ``n`` increments; ``ws_elems`` is the library's
    ``hfem_grid_param_ws_elems``.  grid / mask / ggrid have n + 1 entries (mask: uint8), p / gp / cum have n."""
    return dict(p=n, gp=n, grid=n + 1, ggrid=n + 1, mask=n + 1, initial=n + 1, cum=n, ws=int(ws_elems(n)))


# ------------------------------------------------------------------------------------------------ 1D statement
def elem_index(grid, x, right=False):
    """reference src/models.py:73-74: a point on node k > 0 belongs to the left element, a point on grid[0] to element 0."""
    return (torch.searchsorted(grid, x, right=right) - 1).clamp(0, grid.shape[0] - 2)


def dudx(grid, u_full, x_eval, eps=EPS_H, elem=elem_index):
    """du/dx of the hat interpolation as a differentiable expression of grid and u (examples/example3.py:56 takes it with
    ``autograd.grad(u, xq, create_graph=True)``; this is the same number)."""
    e = elem(grid, x_eval)
    return (u_full[e + 1] - u_full[e]) / (grid[e + 1] - grid[e]).clamp(eps)


def line2_terms(grid, u_full, x_eval):
    """|u_i N1| + |u_j N2| per point: the scale of the rounding error of one interpolated value."""
    e = elem_index(grid, x_eval)
    h = (grid[e + 1] - grid[e]).clamp(EPS_H)
    return (u_full[e] * (grid[e + 1] - x_eval) / h).abs() + (u_full[e + 1] * (x_eval - grid[e]) / h).abs()


def line2_eval_expected(c, req=("grid", "u", "x"), forward=R.line2_forward, dudx_fn=dudx):
    """pred, dudx and the gradients of sum(cot pred) + sum(cot_d dudx) with respect to the inputs named in ``req``
    (None for the others, and for x when nothing depends on it)."""
    grid, u, x = _leaf(c["grid"], "grid" in req), _leaf(c["u"], "u" in req), _leaf(c["x"], "x" in req)
    pred, d = forward(grid, u, x), dudx_fn(grid, u, x)
    out = dict(pred=pred.detach(), dudx=d.detach(), ggrid=None, gu=None, gx=None)
    leaves = [(k, t) for k, t in (("ggrid", grid), ("gu", u), ("gx", x)) if t.requires_grad]
    if leaves:
        s = (pred * c["cot"]).sum() + (d * c["cot_d"]).sum()
        for (k, _), g in zip(leaves, torch.autograd.grad(s, [t for _, t in leaves], allow_unused=True)):
            out[k] = g
    return out


def line2_mse_expected(c, req=("grid", "u"), forward=R.line2_forward):
    grid, u = _leaf(c["grid"], "grid" in req), _leaf(c["u"], "u" in req)
    loss = R.mse_loss(forward(grid, u, c["x"]), c["target"])
    out = dict(loss=loss.detach(), ggrid=None, gu=None)
    leaves = [(k, t) for k, t in (("ggrid", grid), ("gu", u)) if t.requires_grad]
    for (k, _), g in zip(leaves, torch.autograd.grad(loss, [t for _, t in leaves]) if leaves else ()):
        out[k] = g
    return out


def bar_energy_given(grid, u_full, xq, wq, bq, E, forward=R.line2_forward, dudx_fn=dudx):
    """examples/example3.py:59-68 on GIVEN quadrature points, weights and body-force values (all three detached)."""
    return torch.sum(wq * (0.5 * E * dudx_fn(grid, u_full, xq) ** 2 - bq * forward(grid, u_full, xq)))


def bar_terms(c):
    """(sum of the positive, sum of the negative) per-point terms of the bar energy: how much its sum cancels."""
    t = c["wq"] * (0.5 * c["E"] * dudx(c["grid"], c["u"], c["x"]) ** 2 - c["bq"] * R.line2_forward(c["grid"], c["u"], c["x"]))
    return t.clamp(min=0).sum().item(), t.clamp(max=0).sum().item()


def bar_expected(c, forward=R.line2_forward, dudx_fn=dudx):
    grid, u = _leaf(c["grid"], True), _leaf(c["u"], True)
    loss = bar_energy_given(grid, u, c["x"], c["wq"], c["bq"], c["E"], forward, dudx_fn)
    gg, gu = torch.autograd.grad(loss, [grid, u])
    return dict(loss=loss.detach(), ggrid=gg, gu=gu)


def line_case(grid, u, x, seed):
    """One 1D case dict: the leaf grid and nodal values, the points, and everything else derived from them."""
    g = torch.Generator().manual_seed(seed)
    m = x.shape[0]
    return dict(grid=grid, u=u, x=x, cot=torch.randn(m, generator=g, dtype=F64), cot_d=0.1 * torch.randn(m, generator=g, dtype=F64),
                target=torch.sin(6.0 * x), wq=(1.0 + 0.5 * torch.cos(torch.arange(m, dtype=F64))) / m, bq=torch.cos(3.0 * x), E=2.0)


def to32(c):
    """The case a float-row kernel sees, in fp64 (tensors rounded to fp32 and widened; scalars and index tensors as they are)."""
    return {k: round32(v) if isinstance(v, torch.Tensor) and v.dtype == F64 else v for k, v in c.items()}


# ------------------------------------------------------------------------------------------------ 2D statement
def rect_parts(gx, gy, u_full, x_eval):
    """ix, iy, the four shape-function products and the four nodal values of reference src/models.py:183-206."""
    px, py = x_eval[:, 0], x_eval[:, 1]
    ix, iy = elem_index(gx, px.contiguous()), elem_index(gy, py.contiguous())
    hx, hy = (gx[ix + 1] - gx[ix]).clamp(EPS_H), (gy[iy + 1] - gy[iy]).clamp(EPS_H)
    N1x, N2x, N1y, N2y = (gx[ix + 1] - px) / hx, (px - gx[ix]) / hx, (gy[iy + 1] - py) / hy, (py - gy[iy]) / hy
    return dict(ix=ix, iy=iy, hx=hx, hy=hy, N=(N1x * N1y, N2x * N1y, N1x * N2y, N2x * N2y), Nx=(N1x, N2x), Ny=(N1y, N2y),
                u=(u_full[ix, iy], u_full[ix + 1, iy], u_full[ix, iy + 1], u_full[ix + 1, iy + 1]))


def rect_terms(gx, gy, u_full, x_eval):
    """sum of the four |N_x N_y u| per point."""
    p = rect_parts(gx, gy, u_full, x_eval)
    return sum((n * v).abs() for n, v in zip(p["N"], p["u"]))


def rect_gx_terms(gx, gy, u_full, x_eval, cot):
    """[m, 2]: the summed magnitudes of the four terms of d(cot pred)/d(point): the scale of the rounding error of the point
    gradient, which is a difference of nodal values weighted by the other axis' shape functions and may cancel."""
    p = rect_parts(gx, gy, u_full, x_eval)
    (N1x, N2x), (N1y, N2y), (u00, u10, u01, u11) = p["Nx"], p["Ny"], p["u"]
    tx = ((N1y * u00).abs() + (N1y * u10).abs() + (N2y * u01).abs() + (N2y * u11).abs()) / p["hx"]
    ty = ((N1x * u00).abs() + (N2x * u10).abs() + (N1x * u01).abs() + (N2x * u11).abs()) / p["hy"]
    return cot.abs()[:, None] * torch.stack([tx, ty], dim=1)


def rect_eval_expected(c, req=("gx", "gy", "u", "x"), forward=R.rectq4_forward):
    gx, gy, u, x = (_leaf(c[k], k in req) for k in ("gx", "gy", "u", "x"))
    pred = forward(gx, gy, u, x)
    out = dict(pred=pred.detach(), ggx=None, ggy=None, gu=None, gx_eval=None)
    leaves = [(k, t) for k, t in (("ggx", gx), ("ggy", gy), ("gu", u), ("gx_eval", x)) if t.requires_grad]
    if leaves:
        for (k, _), g in zip(leaves, torch.autograd.grad((pred * c["cot"]).sum(), [t for _, t in leaves])):
            out[k] = g
    return out


def rect_mse_expected(c, req=("gx", "gy", "u"), forward=R.rectq4_forward):
    gx, gy, u = (_leaf(c[k], k in req) for k in ("gx", "gy", "u"))
    loss = R.mse_loss(forward(gx, gy, u, c["x"]), c["target"])
    out = dict(loss=loss.detach(), ggx=None, ggy=None, gu=None)
    leaves = [(k, t) for k, t in (("ggx", gx), ("ggy", gy), ("gu", u)) if t.requires_grad]
    if leaves:
        for (k, _), g in zip(leaves, torch.autograd.grad(loss, [t for _, t in leaves])):
            out[k] = g
    return out


def rect_case(gx, gy, x, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(gx=gx, gy=gy, u=torch.randn(gx.shape[0], gy.shape[0], generator=g, dtype=F64), x=x,
                cot=torch.randn(x.shape[0], generator=g, dtype=F64), target=torch.sin(4.0 * x[:, 0]) * torch.cos(3.0 * x[:, 1]))


def sorted_grid(n, seed, lo=0.0, hi=1.0):
    """n sorted random nodes with the ends exactly on lo and hi (n = 2: just the ends)."""
    g = torch.Generator().manual_seed(seed)
    inner = torch.sort(lo + (hi - lo) * (0.05 + 0.9 * torch.rand(n - 2, generator=g, dtype=F64))).values
    return torch.cat([torch.tensor([lo], dtype=F64), inner, torch.tensor([hi], dtype=F64)])


# ------------------------------------------------------------------------------------------------ D: second grid-stride trip
M_TWO_TRIPS = 262144 + 257                  # 1024 blocks x 256 threads cover 262 144 points in one trip


def two_trip_line_case():
    g = torch.Generator().manual_seed(41)
    grid = sorted_grid(17, 42)
    x = -0.05 + 1.1 * torch.rand(M_TWO_TRIPS, generator=g, dtype=F64)
    return line_case(grid, torch.randn(17, generator=g, dtype=F64), x, 43)


def two_trip_rect_case():
    g = torch.Generator().manual_seed(44)
    x = -0.05 + 1.1 * torch.rand(M_TWO_TRIPS, 2, generator=g, dtype=F64)
    return rect_case(sorted_grid(5, 45), sorted_grid(9, 46), x, 47)


# ------------------------------------------------------------------------------------------------ E: node, end, outside points
E_LINE_ELEMS = [0, 0, 0, 0, 1, 2, 3, 3]    # of the eight fixed points below; the eight random ones follow in the host test


def node_line_case():
    """Grid [0, .25, .5, .75, 1]; points left of it, on every node (same fp64 bit patterns), right of it, and 8 random interior
    ones."""
    grid = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], dtype=F64)
    g = torch.Generator().manual_seed(51)
    x = torch.cat([torch.tensor([-0.1, 0.0, 0.1, 0.25, 0.5, 0.75, 1.0, 1.2], dtype=F64),
                   0.01 + 0.98 * torch.rand(8, generator=g, dtype=F64)])
    return line_case(grid, torch.randn(5, generator=g, dtype=F64), x, 52)


RECT_SHAPES = ((2, 2), (2, 9), (9, 2), (5, 9))


def node_rect_case(nx, ny):
    """Points on all four corners, on each edge, on interior grid lines (where the axis has any), outside each side and
    outside a corner, plus 8 random interior points.  Node coordinates are copied from the grids: same bit patterns."""
    gx, gy = sorted_grid(nx, 60 + nx), sorted_grid(ny, 70 + ny)
    g = torch.Generator().manual_seed(80 + 10 * nx + ny)
    a, b = gx[nx // 2 - 1 if nx > 2 else 0].item(), gy[ny // 2 - 1 if ny > 2 else 0].item()     # an interior line (or the low end)
    mx, my = 0.37, 0.61
    pts = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0),                     # corners
           (mx, 0.0), (mx, 1.0), (0.0, my), (1.0, my),                         # edges
           (a, my), (mx, b), (a, b),                                           # grid lines / a node (or the low edges for n = 2)
           (-0.2, my), (1.3, my), (mx, -0.15), (mx, 1.25),                     # outside each side
           (-0.1, -0.3), (1.2, 1.1), (-0.05, 1.4)]                             # outside corners
    if nx > 2:
        pts += [(gx[k].item(), my) for k in range(1, nx - 1)]                  # every interior x line
    if ny > 2:
        pts += [(mx, gy[k].item()) for k in range(1, ny - 1)]                  # every interior y line
    x = torch.cat([torch.tensor(pts, dtype=F64), 0.01 + 0.98 * torch.rand(8, 2, generator=g, dtype=F64)])
    return rect_case(gx, gy, x, 90 + 10 * nx + ny)


# ------------------------------------------------------------------------------------------------ F: the h clamp
TINY = 5e-11                                # below the clamp (1e-10): h is clamped and carries no gradient
F_GRID = [0.0, 0.25, 0.5, 0.5 + TINY, 0.75, 1.0]
F_POINTS = [0.1, 0.5, 0.5 + 2e-11, 0.5 + TINY, 0.6]
F_ELEMS = [0, 1, 2, 2, 3]
DUP_GRID = [0.0, 0.5, 0.5, 1.0]
DUP_POINTS = [0.25, 0.5, 0.75]
DUP_ELEMS = [0, 0, 2]                       # no point lands in the zero-length element 1


def clamp_line_case(dup=False):
    if dup:
        grid, x = torch.tensor(DUP_GRID, dtype=F64), torch.tensor(DUP_POINTS, dtype=F64)
        u = torch.tensor([0.4, -0.9, 1.3, 0.2], dtype=F64)
    else:
        grid, x = torch.tensor(F_GRID, dtype=F64), torch.tensor(F_POINTS, dtype=F64)
        u = torch.tensor([0.3, -1.2, 0.8, 2.0, -0.5, 1.1], dtype=F64)
    return line_case(grid, u, x, 61 + dup)


def clamp_rect_case():
    """4 x 6: the duplicated-node grid on x, the 5e-11 grid on y; 3 x 5 = 15 points."""
    x = torch.tensor([(px, py) for px in DUP_POINTS for py in F_POINTS], dtype=F64)
    return rect_case(torch.tensor(DUP_GRID, dtype=F64), torch.tensor(F_GRID, dtype=F64), x, 63)


def per_point_grads(term, leaves, m):
    """One reference backward pass per point: ``term(q, *leaves)`` is point q's share of the differentiated scalar.
    -> ([sum_q contribution], [sum_q |contribution|]) per leaf; the second is case F's tolerance scale."""
    tot = [torch.zeros_like(t) for t in leaves]
    mag = [torch.zeros_like(t) for t in leaves]
    for q in range(m):
        ls = [_leaf(t, True) for t in leaves]
        for k, g in enumerate(torch.autograd.grad(term(q, *ls), ls, allow_unused=True)):
            if g is not None:
                tot[k] += g
                mag[k] += g.abs()
    return tot, mag


def line_point_terms(c):
    """name -> term(q, grid, u) for the three differentiated scalars of a 1D case (eval with both cotangents, mse, bar)."""
    x, m = c["x"], c["x"].shape[0]

    def ev(q, grid, u):
        s = slice(q, q + 1)
        return (R.line2_forward(grid, u, x[s]) * c["cot"][s] + dudx(grid, u, x[s]) * c["cot_d"][s]).sum()

    def mse(q, grid, u):
        s = slice(q, q + 1)
        return ((R.line2_forward(grid, u, x[s]) - c["target"][s]) ** 2).sum() / m

    def bar(q, grid, u):
        s = slice(q, q + 1)
        return bar_energy_given(grid, u, x[s], c["wq"][s], c["bq"][s], c["E"])

    return dict(eval=ev, mse=mse, bar=bar)


def rect_point_terms(c):
    x, m = c["x"], c["x"].shape[0]

    def ev(q, gx, gy, u):
        s = slice(q, q + 1)
        return (R.rectq4_forward(gx, gy, u, x[s]) * c["cot"][s]).sum()

    def mse(q, gx, gy, u):
        s = slice(q, q + 1)
        return ((R.rectq4_forward(gx, gy, u, x[s]) - c["target"][s]) ** 2).sum() / m

    return dict(eval=ev, mse=mse)


# ------------------------------------------------------------------------------------------------ G: gradient subsets
LINE_EVAL_SUBSETS = (("grid",), ("u",), ("x",), ("grid", "u", "x"))
LINE_MSE_SUBSETS = (("grid",), ("u",), ("grid", "u"))
RECT_EVAL_SUBSETS = (("gx", "gy"), ("u",), ("x",), ("gx", "gy", "u", "x"))
RECT_MSE_SUBSETS = (("gx", "gy"), ("u",), ("gx", "gy", "u"))


def subset_line_case():
    g = torch.Generator().manual_seed(71)
    x = -0.05 + 1.1 * torch.rand(301, generator=g, dtype=F64)
    return line_case(sorted_grid(13, 72), torch.randn(13, generator=g, dtype=F64), x, 73)


def subset_rect_case():
    g = torch.Generator().manual_seed(74)
    x = -0.05 + 1.1 * torch.rand(301, 2, generator=g, dtype=F64)
    return rect_case(sorted_grid(6, 75), sorted_grid(4, 76), x, 77)
