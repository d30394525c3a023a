"""Inputs, sizes and CPU statements for the edge cases of the per-point (csrc/tri3_eval.hip), planless atomic
(tri3_energy.hip, quad4.hip), post-processing (post.hip), row-assembly and row-Adam (optim.hip) kernels, shared by
tests/test_pointwise_cases_host.py and tests/test_gpu_pointwise_edges.py (a plain helper module, not a conftest).

Everything is built deterministically on the CPU in fp64 (seeded ``torch.Generator``) and nothing of the GPU library is
imported.  Expected results come from the project's CPU oracles: ``oracle.ref_chain`` under autograd, ``oracle.quad4``, the
plain-C ``oracle.closed_form`` and the numpy von Mises formulas of tests/test_gpu_post.py.  Added here: a
``numpy.longdouble`` restatement of the per-point TRI3 closed form (forward and backward), the judge of the one
near-degenerate element, and a numpy restatement of one ``torch.optim.Adam`` step on listed rows.

Why the nodal values of the per-point cases are what they are: ``u_h`` is held to rtol 1e-13 at points OUTSIDE their element,
where the three weights have both signs.  Random nodal values would let ``sum_k w_k U_k`` cancel for some of 524 289 points
and turn the bound into a statement about luck, so ``u_positive`` keeps each component within 10 % of one value (and the
Dirichlet value of the model cases of the same sign): |result| >= 0.2 max|term| for every weight in [-0.3, 1.3]^2.
"""
import functools
import itertools

import numpy as np
import torch

from oracle import quad4 as Q4
from oracle import ref_chain as R

F32, F64 = torch.float32, torch.float64
LD = np.longdouble

# ------------------------------------------------------------------------------------------------ bounds of the GPU test
U_RTOL = 1e-13                              # u_h, detJ, ds (tests/test_gpu_parity.py)
GRADU_RTOL, GRADU_ATOL = 1e-11, 1e-16       # per-point grad_u (tests/test_gpu_parity.py)
LOSS_RTOL, GRAD_RTOL = 1e-12, 1e-10         # losses; accumulated gradients relative to max|g|
VM_RTOL = 1e-12                             # von Mises (tests/test_gpu_post.py)
POST_GRADU_RTOL, POST_GRADU_ATOL = 1e-12, 1e-16
SLOPE_RTOL, SLOPE_ATOL = 1e-11, 1e-14       # line2 slopes (tests/test_gpu_post.py)
ADAM_RTOL = 1e-14                           # row Adam against the fp64 formula (tests/test_gpu_parity.py, fused Adam)
DEGENERATE_FACTOR = 8                       # allowance of the near-degenerate element: this x the fp64 oracle's own error

# ------------------------------------------------------------------------------------------------ sizes
# Every cap is (blocks) x (threads per block) of the grid helper named beside it; one item more than the cap is the smallest
# count at which the grid-stride loop of that launch runs a second trip.
BLOCK = 256                                 # kBlockE (tri3_eval.hip), kBlock (tri3_energy.hip), kBlockQ (quad4.hip), post.hip
EVAL_CAP = 2048 * BLOCK                     # grid_e(n): g > 2048 ? 2048 : g                    csrc/tri3_eval.hip
ENERGY_CAP = 256 * 8 * BLOCK                # grid_for(n, cap = 256 * 8)                        csrc/tri3_energy.hip
QUAD4_CAP = 4096 * BLOCK                    # grid_q(n): g > 4096 ? 4096 : g                    csrc/quad4.hip
POST_CAP = 8192 * BLOCK                     # post_grid(n): g > 8192 ? 8192 : g                 csrc/post.hip
POINT_M = (1, 255, 256, 257, EVAL_CAP + 1)
ENERGY_N = (1, 257, ENERGY_CAP + 1)
QUAD4_N = (1, 257, QUAD4_CAP + 1)
POST_N = (1, 256, 257, POST_CAP + 1)
ROW_WIDTHS = (1, 2, 3)
ONE_ELEMENT_M = 4096                        # every point in one element: twelve addresses take all the atomics


def row_counts(width):
    """rows x width crosses EVAL_CAP (scatter / gather launch grid_e(rows * width))."""
    return (0, 1, 257, EVAL_CAP // width + 1)


def slope_nodes(dim_u):
    """n_nodes of hfem_line2_slopes; the last one has (n_nodes - 1) * dim_u > POST_CAP."""
    return (0, 1, 2, 257, POST_CAP // dim_u + 2)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ meshes
NCX, NCY = 6, 4                             # cells; at most about 12 x 9 (the issue's limit for the host oracle's cost)
FLIP_EVERY = 3                              # elements e with e % 3 == 1 are listed clockwise


@functools.lru_cache(maxsize=None)
def tri_mesh():
    """(NCX+1) x (NCY+1) jittered nodes on [0,2] x [0,1], two triangles per cell, every third element clockwise.  ->
    dict(X, conn, edges, boundary_mask, dirichlet_mask); ``edges``: the right side, every edge in both directions;
    ``boundary_mask``: the left, lower and upper sides; ``dirichlet_mask``: the left side."""
    nx, ny = NCX + 1, NCY + 1
    xs, ys = torch.linspace(0, 2, nx, dtype=F64), torch.linspace(0, 1, ny, dtype=F64)
    X = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), dim=-1).reshape(-1, 2)
    X = X + 0.2 * (torch.rand(X.shape, generator=_gen(5), dtype=F64) - 0.5) * torch.tensor([2 / NCX, 1 / NCY], dtype=F64)
    conn = []
    for i, j in itertools.product(range(NCX), range(NCY)):
        n00, n10 = i * ny + j, (i + 1) * ny + j
        conn += [[n00, n10, n10 + 1], [n00, n10 + 1, n00 + 1]]
    conn = torch.tensor(conn)
    flip = torch.arange(conn.shape[0]) % FLIP_EVERY == 1
    conn[flip] = conn[flip][:, [0, 2, 1]]
    right = [[NCX * ny + j, NCX * ny + j + 1] for j in range(NCY)]
    edges = torch.tensor(right + [[b, a] for a, b in right])
    ij = torch.tensor(list(itertools.product(range(nx), range(ny))))
    boundary = (ij[:, 0] == 0) | (ij[:, 1] == 0) | (ij[:, 1] == NCY)   # not the right side: the edges' ds gradient must reach free rows
    return dict(X=X, conn=conn, edges=edges, boundary_mask=boundary, dirichlet_mask=ij[:, 0] == 0)


@functools.lru_cache(maxsize=None)
def quad_mesh():
    """The same nodes as QUAD4 cells (counter-clockwise from the lower left corner); every third cell clockwise."""
    ny = NCY + 1
    conn = []
    for i, j in itertools.product(range(NCX), range(NCY)):
        n00, n10 = i * ny + j, (i + 1) * ny + j
        conn.append([n00, n10, n10 + 1, n00 + 1])
    conn = torch.tensor(conn)
    flip = torch.arange(conn.shape[0]) % FLIP_EVERY == 1
    conn[flip] = conn[flip][:, [0, 3, 2, 1]]
    return dict(X=tri_mesh()["X"], conn=conn)


U_FIXED = 1.5e-3                            # Dirichlet value of the model cases: the sign of both components below


def u_positive(n, seed=11):
    """Nodal values of one sign and within 10 % of each other per component (see the module docstring)."""
    r = torch.rand((n, 2), generator=_gen(seed), dtype=F64)
    return torch.tensor([1e-3, 2e-3], dtype=F64) * (1.0 + 0.1 * r)


def u_strain(X, seed=12):
    """A displacement with a real strain (a linear field plus 5 % noise): energies and von Mises stresses of it are sums
    of positive terms of one magnitude."""
    lin = torch.stack([0.3 * X[:, 0] + 0.1 * X[:, 1], -0.2 * X[:, 0] + 0.25 * X[:, 1]], dim=1)
    return 1e-3 * (lin + 0.05 * torch.randn(X.shape, generator=_gen(seed), dtype=F64))


# ------------------------------------------------------------------------------------------------ point sets
VERTICES = [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]
EDGE_MIDPOINTS = [[0.5, 0.5], [0.0, 0.5], [0.5, 0.0]]
CENTROID = [[1 / 3, 1 / 3]]
OUTSIDE = [[-0.25, 0.5], [1.25, -0.125], [0.75, 0.75], [-0.3, -0.3]]     # a negative weight each; the last has zeta = 1.6 > 1
SPECIAL = VERTICES + EDGE_MIDPOINTS + CENTROID + OUTSIDE
XI_SPECIAL = [0.0, 1.0, 0.5, 0.3125, -0.25, 1.5]                          # EDGE2: both ends, interior, outside on both sides


def barycentric(x_eval):
    return torch.cat([x_eval, 1.0 - x_eval.sum(dim=1, keepdim=True)], dim=1)


def random_points(m, seed):
    """Points of [-0.3, 1.3]^2: inside and outside their element."""
    return -0.3 + 1.6 * torch.rand((m, 2), generator=_gen(seed), dtype=F64)


def _cotangents(m, seed):
    g = _gen(seed)
    return dict(cu=torch.randn((m, 2), generator=g, dtype=F64), cd=torch.randn((m,), generator=g, dtype=F64),
                cg=torch.randn((m, 2, 2), generator=g, dtype=F64))


TRI3_IDS = ("arange", "multiset", "one", "special")
ONE_ELEMENT = 7                             # a clockwise element (7 % 3 == 1)


@functools.lru_cache(maxsize=None)
def tri3_case(ids, m=None):
    """One per-point TRI3 case -> dict(X, U, conn, x_eval, elem_id, cu, cd, cg).  ``ids``: "arange" (every element once),
    "multiset" (m random ids with repeats), "one" (m points in element ONE_ELEMENT), "special" (SPECIAL in every element)."""
    mesh = tri_mesh()
    ne = mesh["conn"].shape[0]
    if ids == "arange":
        elem_id, x_eval = torch.arange(ne), random_points(ne, 21)
    elif ids == "multiset":
        elem_id = torch.randint(0, ne, (m,), generator=_gen(22 + m))
        x_eval = random_points(m, 23 + m)
    elif ids == "one":
        elem_id, x_eval = torch.full((m,), ONE_ELEMENT), random_points(m, 24)
    elif ids == "special":
        elem_id = torch.arange(ne).repeat_interleave(len(SPECIAL))
        x_eval = torch.tensor(SPECIAL, dtype=F64).repeat(ne, 1)
    else:
        raise ValueError(ids)
    return dict(X=mesh["X"], U=u_positive(mesh["X"].shape[0]), conn=mesh["conn"], x_eval=x_eval, elem_id=elem_id,
                **_cotangents(elem_id.shape[0], 25 + elem_id.shape[0]))


def tri3_expected(c, convention="reference", cots=("cu", "cd", "cg")):
    """``oracle.ref_chain.tri3_forward`` and autograd of sum(out * cot) over the cotangents named in ``cots`` ->
    dict(u_h, detJ, grad_u, gX, gU); no cotangent at all: zero gradients."""
    X, U = _leaf(c["X"]), _leaf(c["U"])
    u_h, detJ, grad_u = R.tri3_forward(X, U, c["conn"], c["x_eval"], c["elem_id"], convention)
    out = dict(u_h=u_h.detach(), detJ=detJ.detach(), grad_u=grad_u.detach(), gX=torch.zeros_like(X), gU=torch.zeros_like(U))
    terms = [(o * c[k]).sum() for k, o in (("cu", u_h), ("cd", detJ), ("cg", grad_u)) if k in cots]
    if terms:
        sum(terms).backward()
        out["gX"] = X.grad if X.grad is not None else out["gX"]       # u_h alone does not depend on X
        out["gU"] = U.grad if U.grad is not None else out["gU"]       # nor detJ alone on U
    return out


@functools.lru_cache(maxsize=None)
def tri3_expected_cached(ids, m, convention):
    return tri3_expected(tri3_case(ids, m), convention)


COT_SUBSETS = [s for k in range(4) for s in itertools.combinations(("cu", "cd", "cg"), k)]     # all eight, () first


# ------------------------------------------------------------------------------------------------ the near-degenerate element
DEGENERATE_HEIGHT = 1e-6


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """One element of base 1 and height 1e-6 (aspect 1e6, det = 4e-6 of the product of the two edges at its last node),
    turned by 0.7 rad so that a d and b c are both of order 0.2 and det = a d - b c loses ten digits; SPECIAL plus twenty
    random points."""
    base = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.5, DEGENERATE_HEIGHT]], dtype=F64)
    co, si = np.cos(0.7), np.sin(0.7)
    X = base @ torch.tensor([[co, si], [-si, co]], dtype=F64) + torch.tensor([0.3, 0.2], dtype=F64)
    x_eval = torch.cat([torch.tensor(SPECIAL, dtype=F64), random_points(20, 31)])
    m = x_eval.shape[0]
    return dict(X=X, U=u_positive(3, 32), conn=torch.tensor([[0, 1, 2]]), x_eval=x_eval,
                elem_id=torch.zeros(m, dtype=torch.long), **_cotangents(m, 33))


def tri3_closed_form_ld(c, convention="reference", cots=("cu", "cd", "cg")):
    """The closed form csrc/tri3_eval.hip states (forward and hand-derived backward), in ``numpy.longdouble`` on the fp64
    inputs -> dict of longdouble arrays (u_h, detJ, grad_u, gX, gU)."""
    phys = convention == "physical"
    X, U = c["X"].numpy().astype(LD), c["U"].numpy().astype(LD)
    n = c["conn"].numpy()[c["elem_id"].numpy()]
    r = c["x_eval"].numpy().astype(LD)
    m = n.shape[0]
    X0, X1, X2, U0, U1, U2 = X[n[:, 0]], X[n[:, 1]], X[n[:, 2]], U[n[:, 0]], U[n[:, 1]], U[n[:, 2]]
    zeta = 1 - r[:, 0] - r[:, 1]
    u_h = r[:, :1] * U0 + r[:, 1:] * U1 + zeta[:, None] * U2
    a, d = X0[:, 0] - X2[:, 0], X1[:, 1] - X2[:, 1]
    b, cc = X1[:, 0] - X2[:, 0], X0[:, 1] - X2[:, 1]
    if phys:
        b, cc = cc, b
    det = a * d - b * cc
    inv = 1 / det
    g0, g1 = U0 - U2, U1 - U2
    h00, h01 = (g0[:, 0] * d - g1[:, 0] * b) * inv, (g1[:, 0] * a - g0[:, 0] * cc) * inv
    h10, h11 = (g0[:, 1] * d - g1[:, 1] * b) * inv, (g1[:, 1] * a - g0[:, 1] * cc) * inv
    grad_u = np.stack([np.stack([h00, h01], 1), np.stack([h10, h11], 1)], 1)
    zero = np.zeros(m, dtype=LD)
    P = c["cg"].numpy().astype(LD) if "cg" in cots else np.zeros((m, 2, 2), dtype=LD)
    q = c["cu"].numpy().astype(LD) if "cu" in cots else np.zeros((m, 2), dtype=LD)
    cdet = c["cd"].numpy().astype(LD) if "cd" in cots else zero
    P00, P01, P10, P11 = P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1]
    dg0 = np.stack([(P00 * d - P01 * cc) * inv, (P10 * d - P11 * cc) * inv], 1)
    dg1 = np.stack([(P01 * a - P00 * b) * inv, (P11 * a - P10 * b) * inv], 1)
    gu = [dg0 + r[:, :1] * q, dg1 + r[:, 1:] * q, zeta[:, None] * q - (dg0 + dg1)]
    ddet = cdet - (P00 * h00 + P01 * h01 + P10 * h10 + P11 * h11) * inv
    da = (P01 * g1[:, 0] + P11 * g1[:, 1]) * inv + ddet * d
    db = -(P00 * g1[:, 0] + P10 * g1[:, 1]) * inv - ddet * cc
    dc = -(P01 * g0[:, 0] + P11 * g0[:, 1]) * inv - ddet * b
    dd = (P00 * g0[:, 0] + P10 * g0[:, 1]) * inv + ddet * a
    if phys:
        gx = [np.stack([da, db], 1), np.stack([dc, dd], 1), np.stack([-(da + dc), -(db + dd)], 1)]
    else:
        gx = [np.stack([da, dc], 1), np.stack([db, dd], 1), np.stack([-(da + db), -(dc + dd)], 1)]
    gX, gU = np.zeros_like(X), np.zeros_like(U)
    for k in range(3):
        np.add.at(gX, n[:, k], gx[k])
        np.add.at(gU, n[:, k], gu[k])
    return dict(u_h=u_h, detJ=det, grad_u=grad_u, gX=gX, gU=gU)


def max_err_ld(got, want_ld):
    """max |got - want| with the difference taken in longdouble."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(got.astype(LD).reshape(want_ld.shape) - want_ld).max())


# max |oracle.ref_chain (fp64) - longdouble restatement| on degenerate_case(), per convention and quantity, as measured by
# tests/test_pointwise_cases_host.py::test_degenerate_oracle_error_is_the_recorded_one (which holds the measurement to these
# figures).  The GPU's allowance is DEGENERATE_FACTOR x these; nothing here comes from a kernel's output.
DEGENERATE_REF_ERR = {
    "reference": dict(detJ=1.0046e-18, grad_u=3.0342e-11, gX=5.5791e-05, gU=4.7266e-07),
    "physical": dict(detJ=1.0046e-18, grad_u=5.2145e-11, gX=6.6172e-04, gU=7.2264e-06),
}


def degenerate_measured(convention):
    c = degenerate_case()
    ref, ld = tri3_expected(c, convention), tri3_closed_form_ld(c, convention)
    return {k: max_err_ld(ref[k], ld[k]) for k in ("detJ", "grad_u", "gX", "gU")}


# ------------------------------------------------------------------------------------------------ EDGE2 per-point
EDGE2_IDS = ("arange", "multiset", "one", "special")
ONE_EDGE = 5                                # one of the edges listed from top to bottom


@functools.lru_cache(maxsize=None)
def edge2_case(ids, m=None):
    """-> dict(X, U, edges, xi, edge_id, cu, cd); ``cd`` is the cotangent of ds.  xi in [-0.3, 1.3]."""
    mesh = tri_mesh()
    ned = mesh["edges"].shape[0]
    if ids == "arange":
        edge_id = torch.arange(ned)
    elif ids == "multiset":
        edge_id = torch.randint(0, ned, (m,), generator=_gen(41 + m))
    elif ids == "one":
        edge_id = torch.full((m,), ONE_EDGE)
    elif ids == "special":
        edge_id = torch.arange(ned).repeat_interleave(len(XI_SPECIAL))
    else:
        raise ValueError(ids)
    m = edge_id.shape[0]
    xi = torch.tensor(XI_SPECIAL, dtype=F64).repeat(ned) if ids == "special" else random_points(m, 42 + m)[:, 0].contiguous()
    cot = _cotangents(m, 43 + m)
    return dict(X=mesh["X"], U=u_positive(mesh["X"].shape[0]), edges=mesh["edges"], xi=xi, edge_id=edge_id, cu=cot["cu"],
                cd=cot["cd"])


def edge2_expected(c, cots=("cu", "cd")):
    """``oracle.ref_chain.edge2_forward`` and autograd -> dict(u_h, ds, gX, gU)."""
    X, U = _leaf(c["X"]), _leaf(c["U"])
    u_h, ds = R.edge2_forward(X, U, c["edges"], c["xi"].unsqueeze(1), c["edge_id"])
    out = dict(u_h=u_h.detach(), ds=ds.detach(), gX=torch.zeros_like(X), gU=torch.zeros_like(U))
    terms = [(o * c[k]).sum() for k, o in (("cu", u_h), ("cd", ds)) if k in cots]
    if terms:
        sum(terms).backward()
        out["gX"] = X.grad if X.grad is not None else out["gX"]
        out["gU"] = U.grad if U.grad is not None else out["gU"]
    return out


@functools.lru_cache(maxsize=None)
def edge2_expected_cached(ids, m):
    return edge2_expected(edge2_case(ids, m))


def edge2_ds_gradient(c):
    """d sum(cd ds) / dX in closed form: +c (Xj - Xi) / |Xj - Xi| on node j, the opposite on node i."""
    X = c["X"].numpy()
    e = c["edges"].numpy()[c["edge_id"].numpy()]
    r = X[e[:, 1]] - X[e[:, 0]]
    f = (c["cd"].numpy() / np.sqrt((r * r).sum(axis=1)))[:, None] * r
    gX = np.zeros_like(X)
    np.add.at(gX, e[:, 1], f)
    np.add.at(gX, e[:, 0], -f)
    return torch.from_numpy(gX)


# ------------------------------------------------------------------------------------------------ through the model
MODEL_M = 1031                              # five blocks and seven points; ids repeat about twenty times each


@functools.lru_cache(maxsize=None)
def model_case():
    """The mesh with its boundary nodes fixed, the left side Dirichlet (U_FIXED) and the right side's edges; free rows of
    ``u_positive``.  -> dict(mesh pieces, coords_free, u_free, x_eval, elem_id, xi, edge_id, w_u, w_d, w_g, w_s): the weights
    of the scalar loss w_u sum(u_h) + w_d sum(detJ) + w_g sum(grad_u) (edges: w_u sum(u_h) + w_s sum(ds)).  Every cotangent
    then reaches the kernels as an EXPANDED (stride 0) tensor, which the wrapper has to materialise, and each has another
    value: a copy that is overwritten by the next one before the launch shows."""
    mesh = dict(tri_mesh())
    nn, ne, ned = mesh["X"].shape[0], mesh["conn"].shape[0], mesh["edges"].shape[0]
    U = u_positive(nn)
    return dict(mesh, coords_free=mesh["X"][~mesh["boundary_mask"]].clone(), u_free=U[~mesh["dirichlet_mask"]].clone(),
                x_eval=random_points(MODEL_M, 51), elem_id=torch.randint(0, ne, (MODEL_M,), generator=_gen(52)),
                xi=random_points(MODEL_M, 53)[:, :1].contiguous(), edge_id=torch.randint(0, ned, (MODEL_M,), generator=_gen(54)),
                w_u=0.5, w_d=0.75, w_g=-1.125, w_s=-1.25)     # fp32 holds them exactly: the fp32 model gets the same cotangents


def model_expected(c, with_boundary=True, coords_free=None, u_free=None, u_fixed=U_FIXED, convention="reference"):
    """The oracle chain of the model: ``assemble_coords`` / ``assemble_u`` -> ``tri3_forward`` / ``edge2_forward`` ->
    the weighted scalar losses -> autograd.  ``with_boundary=False``: no node is fixed (every coordinate row is a
    parameter).  -> dict(tri=(u_h, detJ, grad_u, g_coords_free, g_u_free), edge=(u_h, ds, g_coords_free, g_u_free))."""
    nn = c["X"].shape[0]
    bmask = c["boundary_mask"] if with_boundary else torch.zeros(nn, dtype=torch.bool)
    xf0 = coords_free if coords_free is not None else (c["coords_free"] if with_boundary else c["X"])
    uf0 = u_free if u_free is not None else c["u_free"]
    out = {}
    for branch in ("tri", "edge"):
        xf, uf = _leaf(xf0), _leaf(uf0)
        X = R.assemble_coords(nn, ~bmask, xf, bmask, c["X"][bmask].to(xf.dtype))
        U = R.assemble_u(nn, ~c["dirichlet_mask"], uf, c["dirichlet_mask"], torch.tensor(u_fixed, dtype=uf.dtype))
        if branch == "tri":
            u_h, detJ, grad_u = R.tri3_forward(X, U, c["conn"], c["x_eval"], c["elem_id"], convention)
            (c["w_u"] * u_h.sum() + c["w_d"] * detJ.sum() + c["w_g"] * grad_u.sum()).backward()
            out[branch] = (u_h.detach(), detJ.detach(), grad_u.detach(), xf.grad, uf.grad)
        else:
            u_h, ds = R.edge2_forward(X, U, c["edges"], c["xi"], c["edge_id"])
            (c["w_u"] * u_h.sum() + c["w_s"] * ds.sum()).backward()
            out[branch] = (u_h.detach(), ds.detach(), xf.grad, uf.grad)
    return out


def quad_model_expected(c):
    """The QUAD4 twin of ``model_expected``'s domain branch (``oracle.quad4.quad4_forward``) on ``quad_mesh()``, the same
    masks, weights and ids (taken modulo the cell count), points of [-0.9, 0.9]^2.  -> (x_eval, elem_id, u_h, detJ, grad_u,
    g_coords_free, g_u_free)."""
    q = quad_mesh()
    nn, nq = c["X"].shape[0], q["conn"].shape[0]
    x_eval, elem_id = 1.8 * torch.rand((MODEL_M, 2), generator=_gen(55), dtype=F64) - 0.9, c["elem_id"] % nq
    xf, uf = _leaf(c["coords_free"]), _leaf(c["u_free"])
    X = R.assemble_coords(nn, ~c["boundary_mask"], xf, c["boundary_mask"], c["X"][c["boundary_mask"]])
    U = R.assemble_u(nn, ~c["dirichlet_mask"], uf, c["dirichlet_mask"], torch.tensor(U_FIXED, dtype=F64))
    u_h, detJ, grad_u = Q4.quad4_forward(X, U, q["conn"], x_eval, elem_id)
    (c["w_u"] * u_h.sum() + c["w_d"] * detJ.sum() + c["w_g"] * grad_u.sum()).backward()
    return x_eval, elem_id, u_h.detach(), detJ.detach(), grad_u.detach(), xf.grad, uf.grad


# ------------------------------------------------------------------------------------------------ planless atomic energies
ENERGY_W = 0.25                             # sum of the order-4 triangle weights as the reference scales them
ENERGY_RANGES = (7, 7, 29)                  # cuts a, a, b: [0,7) [7,7) [7,29) [29,ne) -- uneven, one of them empty


def energy_mat():
    from oracle import closed_form as CF
    return CF.plane_stress()


def energy_bk():
    """A body-force table two orders below the strain energy: the loss stays a sum of positive terms."""
    return 1e3 * torch.randn(6, generator=_gen(61), dtype=F64).numpy()


def repeated(rows, n):
    """n rows: ``rows`` over and over (row i is rows[i % len(rows)])."""
    return rows[torch.arange(n) % rows.shape[0]]


SLICE = 4096


def _sliced(n, one):
    """The plain-C oracle adds its element energies one after the other.  Over 10^6 equal-signed terms that repeat with the
    period of the tiny mesh the roundings of such a sum drift one way: 4.7e-12 (QUAD4, 1 048 577 rows) and 6.5e-13 (TRI3,
    524 289 rows) of the exact sum, as tests/test_pointwise_cases_host.py measures -- more than LOSS_RTOL, which is asked of
    the KERNEL.  So the oracle is called on consecutive slices of SLICE rows (``one(lo, hi) -> (energy, gX, gU)``) and the
    slices are added exactly (``math.fsum``): the same function on the same rows, without the drift."""
    import math
    parts = [one(lo, min(lo + SLICE, n)) for lo in range(0, n, SLICE)]
    return math.fsum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts)


@functools.lru_cache(maxsize=None)
def tri3_energy_expected(n):
    """-> (conn [n,3], loss, gX, gU) of ``closed_form.tri3_energy`` on the mesh's connectivity repeated to n rows."""
    from oracle import closed_form as CF
    mesh = tri_mesh()
    conn = repeated(mesh["conn"], n)
    X, U, rows, mat, bk = mesh["X"].numpy(), u_strain(mesh["X"]).numpy(), conn.numpy(), energy_mat(), energy_bk()
    return (conn,) + _sliced(n, lambda lo, hi: CF.tri3_energy(X, U, rows[lo:hi], mat, ENERGY_W, bk))


@functools.lru_cache(maxsize=None)
def quad4_energy_expected(n):
    from oracle import closed_form as CF
    mesh = quad_mesh()
    conn = repeated(mesh["conn"], n)
    X, U, rows, mat = mesh["X"].numpy(), u_strain(mesh["X"]).numpy(), conn.numpy(), energy_mat()
    return (conn,) + _sliced(n, lambda lo, hi: CF.quad4_energy(X, U, rows[lo:hi], mat))


def edge_tractions(n):
    """T[n][4] = {Ti.x, Ti.y, Tj.x, Tj.y}: positive, every row different (row g = base x (1 + g / n))."""
    base = torch.tensor([2e5, 3e4, 1.5e5, 5e4], dtype=F64)
    return base[None, :] * (1.0 + torch.arange(n, dtype=F64)[:, None] / n) * torch.tensor([1.0, 1.1, 0.9, 1.2], dtype=F64)


@functools.lru_cache(maxsize=None)
def edge2_energy_expected(n):
    """-> (edges [n,2], T [n,4], loss = -work, gX, gU) of ``closed_form.edge2_energy(T=...)`` on the edges repeated to n rows
    (positive U, positive T: the work is a sum of positive terms)."""
    from oracle import closed_form as CF
    mesh = tri_mesh()
    X, U = mesh["X"].numpy(), u_positive(mesh["X"].shape[0]).numpy()
    edges, T = repeated(mesh["edges"], n), edge_tractions(n)
    rows, Tn = edges.numpy(), T.numpy()

    def one(lo, hi):
        gX, gU = np.zeros_like(X), np.zeros_like(U)
        return CF.edge2_energy(X, U, rows[lo:hi], T=Tn[lo:hi], gX=gX, gU=gU), gX, gU
    work, gX, gU = _sliced(n, one)
    return edges, T, -work, gX, gU


# ------------------------------------------------------------------------------------------------ post-processing
POST_E, POST_NU = 3.0, 0.45


def von_mises_formula(g, E, nu):
    """tests/test_gpu_post.py's numpy restatement of the reference's plot_von_mises, on grad_u [n,2,2]."""
    exx, eyy, exy = g[:, 0, 0], g[:, 1, 1], 0.5 * (g[:, 0, 1] + g[:, 1, 0])
    sxx, syy, sxy = E / (1 - nu ** 2) * (exx + nu * eyy), E / (1 - nu ** 2) * (eyy + nu * exx), E / (1 + nu) * exy
    return np.sqrt(sxx ** 2 - sxx * syy + syy ** 2 + 3 * sxy ** 2)


@functools.lru_cache(maxsize=None)
def von_mises_base(kind):
    """-> (X, U, conn, grad_u [ne,2,2], vm [ne]) of the tiny mesh: the centroid (TRI3) / cell-centre (QUAD4) chain of the
    oracle, then the numpy formulas with POST_E, POST_NU."""
    mesh = tri_mesh() if kind == "tri3" else quad_mesh()
    X, conn = mesh["X"], mesh["conn"]
    U, ne = u_strain(X), conn.shape[0]
    if kind == "tri3":
        _, _, g = R.tri3_forward(X, U, conn, torch.tensor(CENTROID, dtype=F64).expand(ne, 2), torch.arange(ne))
    else:
        _, _, g = Q4.quad4_forward(X, U, conn, torch.zeros((ne, 2), dtype=F64), torch.arange(ne))
    g = g.numpy()
    return X, U, conn, g, von_mises_formula(g, POST_E, POST_NU)


def slopes_case(n_nodes, dim_u):
    """A non-uniform grid (steps of 0.5 .. 1.5) and values u [n_nodes, dim_u] -> (grid, u, expected slopes)."""
    g = _gen(71 + dim_u)
    grid = torch.cumsum(0.5 + torch.rand(max(n_nodes, 1), generator=g, dtype=F64), dim=0)[:n_nodes]
    u = torch.randn((n_nodes, dim_u), generator=g, dtype=F64)
    want = (u[1:] - u[:-1]) / (grid[1:] - grid[:-1])[:, None] if n_nodes >= 2 else torch.zeros((0, dim_u), dtype=F64)
    return grid, u, want


def slopes_by_autograd(grid, u):
    """The reference's compute_du_dx_per_element as tests/test_gpu_post.py states it: autograd of the 1D forward at every
    element midpoint, one component at a time."""
    cols = []
    for k in range(u.shape[1]):
        xm = (0.5 * (grid[:-1] + grid[1:])).clone().requires_grad_(True)
        cols.append(torch.autograd.grad(R.line2_forward(grid, u[:, k].contiguous(), xm).sum(), xm)[0])
    return torch.stack(cols, dim=1)


# ------------------------------------------------------------------------------------------------ row assembly
def rows_case(rows, width, n_extra=0):
    """-> (src [rows, width], idx: a random permutation of rows + n_extra destinations cut to rows, int32)."""
    g = _gen(81 + rows + width)
    src = torch.randn((rows, width), generator=g, dtype=F64)
    idx = torch.randperm(rows + n_extra, generator=g)[:rows].to(torch.int32)
    return src, idx


# ------------------------------------------------------------------------------------------------ row Adam
ADAM_N, ADAM_LISTED, ADAM_STEPS = 300, 137, 5
ADAM_HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)


@functools.lru_cache(maxsize=None)
def adam_case():
    """p, m, v [ADAM_N, 2], ADAM_LISTED listed rows in random order, ADAM_STEPS gradients.  No step cancels: |p| >= 0.5
    against 0.05 of total movement, every gradient keeps its entry's sign and m starts with that sign, so "1e-14 relative"
    can be asked of every entry."""
    g = _gen(91)
    sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).to(F64)
    p = sign((ADAM_N, 2)) * (0.5 + torch.rand((ADAM_N, 2), generator=g, dtype=F64))
    g_base = sign((ADAM_N, 2)) * (0.2 + torch.rand((ADAM_N, 2), generator=g, dtype=F64))
    m, v = 0.2 * g_base, 0.5 * g_base * g_base
    grads = [g_base * (1.0 + 0.3 * np.cos(1.7 * k)) * (0.8 + 0.4 * torch.rand((ADAM_N, 2), generator=g, dtype=F64))
             for k in range(ADAM_STEPS)]
    rows = torch.randperm(ADAM_N, generator=g)[:ADAM_LISTED].to(torch.int32)
    return dict(p=p, m=m, v=v, grads=grads, rows=rows)


def adam_rows_numpy(p, g, m, v, rows, step, lr, beta1, beta2, eps):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on the listed rows, in torch's association:
    m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, 1 - b2); p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))."""
    p, m, v = p.copy(), m.copy(), v.copy()
    r = np.asarray(rows, dtype=np.int64)
    m[r] = m[r] + (1.0 - beta1) * (g[r] - m[r])
    v[r] = v[r] * beta2 + (1.0 - beta2) * (g[r] * g[r])
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p[r] = p[r] - (lr / bc1) * (m[r] / (np.sqrt(v[r]) / np.sqrt(bc2) + eps))
    return p, m, v
