"""The cases of tests/line_rect_cases.py pinned by conditions they must satisfy on their own, so that the GPU test
(tests/test_gpu_line_rect_edges.py) cannot pass or fail for the wrong reason: no increment on the softplus knife edge, every
point on a node bit for bit or well away from all of them, every grid spacing clear of the ``h`` clamp or deliberately under
it, and -- the mutation checks -- each case moves its expected values by at least 100 x the GPU test's tolerance when the
rule it is there for is changed in a copy of the statement.  No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

import line_rect_cases as K
from oracle import ref_chain as R

F64 = torch.float64
MUTATION_FACTOR = 100.0


# ------------------------------------------------------------------------------------------------ copies with one rule changed
def grid_param_ge20(increments, x0, xN):
    """R.grid_param with softplus taking ``x >= 20`` as linear (torch: ``x > 20``)."""
    inc = torch.clamp(torch.where(increments == 20.0, increments, F.softplus(increments)), min=1e-6)
    cum = torch.cumsum(inc, dim=0)
    return torch.cat([x0, x0 + (xN - x0) * cum / cum[-1]], dim=0)


def line2_forward_right(grid, u_full, x_eval, eps=1e-10):
    """R.line2_forward with ``searchsorted(right=True)``: a point on a node goes to the RIGHT element."""
    e = K.elem_index(grid, x_eval, right=True)
    x_i, x_j, u_i, u_j = grid[e], grid[e + 1], u_full[e], u_full[e + 1]
    return u_i * ((x_j - x_eval) / (x_j - x_i).clamp(eps)) + u_j * ((x_eval - x_i) / (x_j - x_i).clamp(eps))


dudx_right = functools.partial(K.dudx, elem=functools.partial(K.elem_index, right=True))


def line2_forward_noclamp(grid, u_full, x_eval):
    """R.line2_forward without the ``h`` clamp (and so with the gradient through ``h`` that the clamp stops)."""
    e = K.elem_index(grid, x_eval)
    x_i, x_j, u_i, u_j = grid[e], grid[e + 1], u_full[e], u_full[e + 1]
    return u_i * ((x_j - x_eval) / (x_j - x_i)) + u_j * ((x_eval - x_i) / (x_j - x_i))


dudx_noclamp = functools.partial(K.dudx, eps=-float("inf"))


def rectq4_forward_noclamp(gx, gy, u_full, x_eval):
    return R.rectq4_forward(gx, gy, u_full, x_eval, eps=-float("inf"))


def rectq4_forward_nx_stride(gx, gy, u_full, x_eval, eps=1e-10):
    """R.rectq4_forward reading ``u`` as a flat array with row stride nx in place of ny (wrapped into the array, where the
    wrong stride would leave it)."""
    nx, ny = gx.shape[0], gy.shape[0]
    p = K.rect_parts(gx, gy, u_full, x_eval)
    flat, ix, iy = u_full.reshape(-1), p["ix"], p["iy"]

    def at(i, j):
        return flat[(i * nx + j) % flat.shape[0]]

    us = (at(ix, iy), at(ix + 1, iy), at(ix, iy + 1), at(ix + 1, iy + 1))
    return sum(n * v for n, v in zip(p["N"], us))


def moved(mutant, expected, tol):
    """How far the mutant's value is from the expected one, in units of the GPU test's tolerance (max over entries with a
    nonzero tolerance)."""
    tol = torch.as_tensor(tol, dtype=F64).expand_as(expected)
    ok = tol > 0
    return ((mutant - expected).abs()[ok] / tol[ok]).max().item()


# ------------------------------------------------------------------------------------------------ the helpers are the statement
def test_added_expressions_agree_with_the_reference_chain():
    """``dudx`` is what autograd gives for d(line2_forward)/dx, and the per-point term helpers add up to the forwards."""
    for c in (K.node_line_case(), K.clamp_line_case(), K.clamp_line_case(dup=True), K.subset_line_case()):
        x = c["x"].clone().requires_grad_(True)
        u = R.line2_forward(c["grid"], c["u"], x)
        e = K.elem_index(c["grid"], c["x"])                                      # autograd: u_j / h - u_i / h, rounded twice
        scale = (c["u"][e].abs() + c["u"][e + 1].abs()) / (c["grid"][e + 1] - c["grid"][e]).clamp(K.EPS_H)
        assert ((torch.autograd.grad(u.sum(), x)[0] - K.dudx(c["grid"], c["u"], c["x"])).abs() <= 4e-16 * scale).all()
        assert (K.line2_terms(c["grid"], c["u"], c["x"]) >= u.detach().abs() * (1 - 1e-15)).all()
        xi, wi = R.interval_gauss(2)
        grid = c["grid"]
        if (grid[1:] - grid[:-1]).min() > 1e-8:
            b = R.example3_body_force
            with torch.no_grad():
                xq = (0.5 * (grid[1:] - grid[:-1])[:, None] * xi + 0.5 * (grid[1:] + grid[:-1])[:, None])
                wq = 0.5 * (grid[1:] - grid[:-1])[:, None] * wi
            got = K.bar_energy_given(grid, c["u"], xq, wq, b(xq), 3.0)
            want = R.bar_energy(grid, c["u"], xi, wi, b, 3.0)                    # example 3's own quadrature, same numbers
            assert abs(got.item() - want.item()) <= 1e-14 * abs(want.item())
    for c in (K.node_rect_case(5, 9), K.clamp_rect_case(), K.subset_rect_case()):
        p = K.rect_parts(c["gx"], c["gy"], c["u"], c["x"])
        assert torch.equal(sum(n * v for n, v in zip(p["N"], p["u"])), R.rectq4_forward(c["gx"], c["gy"], c["u"], c["x"]))


# ------------------------------------------------------------------------------------------------ conditions
def test_no_increment_on_the_softplus_knife_edge():
    assert abs(K.SOFTPLUS_KNIFE + 13.8155) < 1e-4
    cases = [K.grid_param_case(n, False) for n in K.ONE_BLOCK_N + (K.ONE_BLOCK_ABI_N,)] + [K.grid_param_long_case()]
    for c in cases:
        for p in (c["p"], K.round32(c["p"])):
            assert (p - K.SOFTPLUS_KNIFE).abs().min() >= 1e-3
            sp = F.softplus(p)
            assert ((sp < 0.6e-6) | (sp > 2e-6)).all()          # -14.5 gives 5.04e-7 (clamped), -13 gives 2.26e-6 (free)
    # the counts of clamped rows (exactly zero gradient) the issue lists
    for n, zeros in ((11, 2), (1023, 186), (2048, 374)):
        grid, gp = K.grid_param_expected(K.grid_param_case(n, False))
        assert int((gp == 0).sum()) == zeros and grid[-1].item() == K.XN and torch.isfinite(grid).all() and torch.isfinite(gp).all()


def test_one_block_sizes_reach_every_chunk_shape():
    """chunk = ceil(n / 1024): 1 up to 1024, 2 up to 2048 (idle threads from 1025, a short last chunk at 2047), 5 at 4097."""
    chunk = lambda n: (n + 1023) // 1024
    assert [chunk(n) for n in K.ONE_BLOCK_N] == [1, 1, 1, 1, 1, 2, 2, 2] and chunk(K.ONE_BLOCK_ABI_N) == 5
    assert -(-K.ONE_BLOCK_ABI_N // 5) == 820                                     # threads 820.. are idle
    assert 2047 % 2 == 1 and (K.WS_LONG_N + 1023) // 1024 == 1025                # short last chunk; nb > 1024
    assert K.M_TWO_TRIPS > 1024 * 256 and K.M_TWO_TRIPS % 256 != 0


def _node_or_clear(grid, x):
    d = (x[:, None] - grid[None, :]).abs()
    assert ((d == 0) | (d >= 1e-12)).all()


def test_every_point_is_on_a_node_or_clear_of_all_nodes():
    for c in (K.node_line_case(), K.clamp_line_case(), K.clamp_line_case(dup=True)):
        _node_or_clear(c["grid"], c["x"])
    _node_or_clear(K.round32(K.node_line_case()["grid"]), K.round32(K.node_line_case()["x"]))
    rects = [K.node_rect_case(nx, ny) for nx, ny in K.RECT_SHAPES]
    for c in rects + [K.to32(c) for c in rects] + [K.clamp_rect_case()]:
        _node_or_clear(c["gx"], c["x"][:, 0])
        _node_or_clear(c["gy"], c["x"][:, 1])


def test_element_of_each_point():
    """A point on a node belongs to the left element, a point on grid[0] to element 0, points outside to the end elements."""
    c = K.node_line_case()
    assert K.elem_index(c["grid"], c["x"]).tolist() == K.E_LINE_ELEMS + E_LINE_RANDOM_ELEMS
    assert (c["x"][[1, 3, 4, 5, 6]] == c["grid"]).all()                           # on the nodes bit for bit
    c = K.clamp_line_case()
    assert K.elem_index(c["grid"], c["x"]).tolist() == K.F_ELEMS == [0, 1, 2, 2, 3]
    assert c["x"][3] == c["grid"][3] and c["x"][1] == c["grid"][2]
    c = K.clamp_line_case(dup=True)
    assert K.elem_index(c["grid"], c["x"]).tolist() == K.DUP_ELEMS == [0, 0, 2]
    for nx, ny in K.RECT_SHAPES:
        c = K.node_rect_case(nx, ny)
        p = K.rect_parts(c["gx"], c["gy"], c["u"], c["x"])
        # corners (0,0) (1,0) (0,1) (1,1); then the four outside-a-side points
        assert p["ix"][:4].tolist() == [0, nx - 2, 0, nx - 2] and p["iy"][:4].tolist() == [0, 0, ny - 2, ny - 2]
        assert p["ix"][11:13].tolist() == [0, nx - 2] and p["iy"][13:15].tolist() == [0, ny - 2]
        on_x = (c["x"][:, 0][:, None] == c["gx"][None, :]).any(1)
        on_y = (c["x"][:, 1][:, None] == c["gy"][None, :]).any(1)
        assert int(on_x.sum()) >= 6 + max(0, nx - 2) and int(on_y.sum()) >= 6 + max(0, ny - 2)
        assert set(p["ix"].tolist()) == set(range(nx - 1)) and set(p["iy"].tolist()) == set(range(ny - 1))
    c = K.clamp_rect_case()
    p = K.rect_parts(c["gx"], c["gy"], c["u"], c["x"])
    assert p["ix"].tolist() == [e for e in K.DUP_ELEMS for _ in K.F_ELEMS] and p["iy"].tolist() == K.F_ELEMS * 3


E_LINE_RANDOM_ELEMS = [3, 2, 0, 3, 0, 0, 3, 2]   # of the eight seeded random points (0.8899.., 0.5691.., 0.0941.., ...)


def test_grid_spacings_are_clear_of_the_h_clamp_or_deliberately_under_it():
    lines = [K.node_line_case(), K.clamp_line_case(), K.clamp_line_case(dup=True), K.subset_line_case(), K.two_trip_line_case()]
    rects = [K.node_rect_case(nx, ny) for nx, ny in K.RECT_SHAPES] + [K.clamp_rect_case(), K.subset_rect_case(), K.two_trip_rect_case()]
    grids = [c["grid"] for c in lines] + [c[k] for c in rects for k in ("gx", "gy")]
    grids += [K.round32(g) for g in grids if (g[1:] - g[:-1]).min() > 1e-8]       # the float rows of every case but F
    tiny = 0
    for g in grids:
        s = g[1:] - g[:-1]
        is_tiny = (s - K.TINY).abs() <= 1.2e-16                                  # 5e-11 as the grid near 0.5 can hold it
        assert ((s >= 1e-8) | (s == 0) | is_tiny).all()
        tiny += int(is_tiny.sum())
    assert tiny == 2 and K.TINY < K.EPS_H                                        # the 1D and the rect clamp cases
    assert len(K.clamp_line_case()["x"]) <= 16 and len(K.clamp_rect_case()["x"]) <= 16
    # the issue's reading of case F: the point 0.5 + 2e-11 sits in the 5e-11 element, where N1 + N2 = 0.5
    c = K.clamp_line_case()
    ones = torch.ones_like(c["u"])
    assert abs(R.line2_forward(c["grid"], ones, c["x"])[2].item() - 0.5) < 1e-5


def test_loss_sums_do_not_cancel():
    """LOSS_RTOL is relative to the loss: the bar energy's positive and negative terms must not cancel it away."""
    for c in (K.two_trip_line_case(), K.node_line_case(), K.clamp_line_case(), K.clamp_line_case(dup=True), K.subset_line_case()):
        pos, neg = K.bar_terms(c)
        assert abs(pos + neg) >= 0.1 * (pos - neg), (pos, neg)


def test_two_trip_points_extrapolate_at_both_ends():
    c = K.two_trip_line_case()
    assert c["x"].shape[0] == K.M_TWO_TRIPS and c["grid"].shape[0] == 17
    assert 1000 < int((c["x"] < 0).sum()) and 1000 < int((c["x"] > 1).sum())
    assert c["x"][262144:].shape[0] == 257                                       # the second trip's share
    c = K.two_trip_rect_case()
    assert (c["gx"].shape[0], c["gy"].shape[0]) == (5, 9)
    assert (c["x"].min(0).values < 0).all() and (c["x"].max(0).values > 1).all()


# ------------------------------------------------------------------------------------------------ mutation checks
@pytest.mark.parametrize("use_mask", [False, True])
def test_mutation_softplus_threshold_moves_the_small_grid(use_mask):
    c = K.grid_param_case(11, use_mask)
    assert (c["p"] == 20.0).sum() == 1
    grid, _ = K.grid_param_expected(c)
    mut, _ = K.grid_param_expected(c, grid_param_ge20)
    m = moved(mut, grid, K.grid_tol(grid, 11))
    print(f"softplus >= 20, n = 11: grid moves {(mut - grid).abs().max().item():.3e} = {m:.0f} x tolerance")
    assert m >= MUTATION_FACTOR


def test_mutation_searchsorted_right_moves_the_point_and_grid_gradients():
    c = K.node_line_case()
    want = K.line2_eval_expected(c)
    mut = K.line2_eval_expected(c, forward=line2_forward_right, dudx_fn=dudx_right)
    m_gx = moved(mut["gx"], want["gx"], K.POINT_RTOL * want["gx"].abs())
    m_gg = moved(mut["ggrid"], want["ggrid"], K.GRAD_RTOL * want["ggrid"].abs().max())
    print(f"searchsorted(right=True), case E: gx_eval moves {m_gx:.2e} x, grid gradient {m_gg:.2e} x tolerance")
    assert m_gx >= MUTATION_FACTOR and m_gg >= MUTATION_FACTOR
    for name, fn in (("mse", K.line2_mse_expected), ("bar", K.bar_expected)):
        w = fn(c)
        kw = dict(forward=line2_forward_right) if name == "mse" else dict(forward=line2_forward_right, dudx_fn=dudx_right)
        assert moved(fn(c, **kw)["ggrid"], w["ggrid"], K.GRAD_RTOL * w["ggrid"].abs().max()) >= MUTATION_FACTOR, name


def test_mutation_no_h_clamp_moves_pred_and_the_grid_gradient():
    c = K.clamp_line_case()
    want = K.line2_eval_expected(c)
    mut = K.line2_eval_expected(c, forward=line2_forward_noclamp, dudx_fn=dudx_noclamp)
    _, mag = K.per_point_grads(K.line_point_terms(c)["eval"], [c["grid"], c["u"]], c["x"].shape[0])
    m_pred = moved(mut["pred"], want["pred"], K.POINT_RTOL * K.line2_terms(c["grid"], c["u"], c["x"]))
    m_gg = moved(mut["ggrid"], want["ggrid"], K.CLAMP_RTOL * mag[0])
    print(f"no h clamp, case F: pred moves {m_pred:.2e} x, grid gradient {m_gg:.2e} x tolerance; max |ggrid| "
          f"{want['ggrid'].abs().max().item():.2e}")
    assert m_pred >= MUTATION_FACTOR and m_gg >= MUTATION_FACTOR
    assert want["ggrid"].abs().max() > 1e9                                       # nine orders above the other cases
    c = K.clamp_rect_case()
    want, mut = K.rect_eval_expected(c), K.rect_eval_expected(c, forward=rectq4_forward_noclamp)
    _, mag = K.per_point_grads(K.rect_point_terms(c)["eval"], [c["gx"], c["gy"], c["u"]], c["x"].shape[0])
    assert moved(mut["pred"], want["pred"], K.POINT_RTOL * K.rect_terms(c["gx"], c["gy"], c["u"], c["x"])) >= MUTATION_FACTOR
    assert moved(mut["ggy"], want["ggy"], K.CLAMP_RTOL * mag[1]) >= MUTATION_FACTOR


@pytest.mark.parametrize("nx,ny", [s for s in K.RECT_SHAPES if s != (2, 2)])
def test_mutation_row_stride_moves_the_rect_pred(nx, ny):
    c = K.node_rect_case(nx, ny)
    want = K.rect_eval_expected(c)["pred"]
    mut = K.rect_eval_expected(c, forward=rectq4_forward_nx_stride)["pred"]
    m = moved(mut, want, K.POINT_RTOL * K.rect_terms(c["gx"], c["gy"], c["u"], c["x"]))
    print(f"u[ix * nx + iy], {nx} x {ny}: pred moves {m:.2e} x tolerance")
    assert m >= MUTATION_FACTOR


def test_per_point_contributions_add_up_to_the_gradient():
    """Case F's tolerance scale comes from one backward pass per point; their sum is the gradient of the whole scalar."""
    for c in (K.clamp_line_case(), K.clamp_line_case(dup=True)):
        want = K.line2_eval_expected(c, req=("grid", "u"))
        tot, mag = K.per_point_grads(K.line_point_terms(c)["eval"], [c["grid"], c["u"]], c["x"].shape[0])
        for t, m, w in zip(tot, mag, (want["ggrid"], want["gu"])):
            assert ((t - w).abs() <= 1e-14 * m).all() and (m >= w.abs() * (1 - 1e-14)).all()


# ------------------------------------------------------------------------------------------------ buffer sizes
def test_abi_buffer_sizes():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    L = _lib.lib()
    for n in K.ONE_BLOCK_N + K.WS_SMALL_N + (K.ONE_BLOCK_ABI_N, K.WS_LONG_N):
        s = K.grid_param_buffer_sizes(n, L.hfem_grid_param_ws_elems)
        nb = (n + 1023) // 1024
        assert s == dict(p=n, gp=n, grid=n + 1, ggrid=n + 1, mask=n + 1, initial=n + 1, cum=n, ws=n + 2 * nb + 8)
        assert s["ws"] >= n + 2 * nb + 2                                          # backward: suf[n], asum[nb], dsum[nb], 2 scalars
