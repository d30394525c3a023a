"""The one kernel frame of the mesh-validity entry points (csrc/hfem_mesh_dev.h, csrc/mesh_guard.hip) at its edge shapes,
through the C ABI on hand-built arrays: ne = 0 (no element launch), 1 (a single lane), 256 (exactly one full workgroup) and 257
(a workgroup and a one-thread tail), both element kinds, all five entry points of a kind, fp64 and fp32 rows.  Fixed rows in the
x and in the u row map, the free rows stored in reverse order; the per-element outputs once non-null and once null; every
output pre-filled with a sentinel.  References: the numpy closed forms and the CPU autograd barrier of the host test modules,
at the tolerances of test_gpu_radapt.py, test_gpu_radapt_quad4.py and test_gpu_hyper_radapt.py (1e-13 relative for the measure
and J, 1e-12 for the bounds, 1e-11 for the barrier, whose atomics reorder the sum); a summary minimum is the minimum of the
per-element output to the bit."""
import math

import numpy as np
import pytest
import torch

from test_hyper_radapt_host import (barrier_torch, det_f_np, hyper_step_bound_np, quad4_corner_ratios_np,
                                    quad4_hyper_step_bound_np)
from test_radapt_host import _measure_np, step_bound_np
from test_radapt_quad4_host import quad4_measure_np, quad4_step_bound_np

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")
SENTINEL = -7.0


def _row_map(fixed):
    """The row map of nodes with the mask `fixed`: fixed rows in node order, the free rows stored in reverse order."""
    src = np.empty(fixed.size, dtype=np.int32)
    src[fixed] = -1 - np.arange(int(fixed.sum()))
    nfree = int((~fixed).sum())
    src[~fixed] = nfree - 1 - np.arange(nfree)
    return src


def _rows(src, V):
    """(free rows, fixed rows) of the values V [nn, 2] by node id under the row map src."""
    free = np.empty((int((src >= 0).sum()), 2))
    free[src[src >= 0]] = V[src >= 0]
    return free, V[src < 0].copy()


def _strip(kind, ne, seed):
    """A hand-built strip of `ne` elements over the nodes (i, j), i = 0.., j = 0, 1 (id 2 i + j), jittered by +-0.2: cells
    numbered counter-clockwise, or each cell cut into two counter-clockwise triangles.  Every third node is a fixed x row and
    every fourth, from node 1, a fixed u row.  -> (conn [ne, npe] int32, x_src, u_src, X [nn, 2], U [nn, 2]) with a smooth
    displacement field U (det F between about 0.6 and 1.5)."""
    rng = np.random.default_rng(seed)
    cells = ne if kind == "quad4" else (ne + 1) // 2
    nn = 2 * (cells + 1)
    i, j = np.divmod(np.arange(nn), 2)
    X = np.stack([i.astype(float), j.astype(float)], axis=1) + rng.uniform(-0.2, 0.2, size=(nn, 2))
    k = np.arange(cells)
    a, b, c, d = 2 * k, 2 * k + 2, 2 * k + 3, 2 * k + 1
    if kind == "quad4":
        conn = np.stack([a, b, c, d], axis=1)
    else:
        conn = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3)[:ne]
    U = np.stack([0.2 * np.sin(1.3 * X[:, 0] + 0.4 * X[:, 1]), 0.16 * np.cos(1.1 * X[:, 0]) * X[:, 1]], axis=1)
    return conn.astype(np.int32), _row_map(np.arange(nn) % 3 == 0), _row_map(np.arange(nn) % 4 == 1), X, U


def _measures(kind, X, R, U, conn):
    """(q, ratio, inverted, J), each [ne], of the CPU closed forms for rows by node id."""
    if kind == "quad4":
        return quad4_measure_np(X[conn], R[conn]) + (quad4_corner_ratios_np(X[conn], U[conn]).min(axis=1),)
    q, r = _measure_np(X, R, conn)
    return q, r, ~(q > 0.0), det_f_np(X[conn], U[conn])


def _bounds(kind, X, U, D, conn, eta):
    """(the step bound, the det F-safe step bound) of the CPU closed forms: the minimum over the elements."""
    small, hyper = (quad4_step_bound_np, quad4_hyper_step_bound_np) if kind == "quad4" else (step_bound_np, hyper_step_bound_np)
    return small(X[conn], D[conn], eta)[0].min(), hyper(X[conn], U[conn], D[conn], eta)[0].min()


@pytest.mark.parametrize("ne", [0, 1, 256, 257])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_c_abi_on_hand_built_arrays_with_fixed_rows(kind, ne):
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    conn, x_src, u_src, X, U = _strip(kind, max(ne, 1), seed=ne)
    conn = conn[:ne]
    rng = np.random.default_rng(100 + ne)
    Xref = X + rng.uniform(-0.05, 0.05, size=X.shape)
    x_free, x_fixed = _rows(x_src, X)
    u_free, u_fixed = _rows(u_src, U)
    # directions by x_free row: a random one at both shares eta, and the displacement field itself, along which det F falls
    # faster than the reference area where u compresses
    directions = [("random", rng.normal(size=x_free.shape), 0.25), ("random", rng.normal(size=x_free.shape), 0.6),
                  ("along u", _rows(x_src, U)[0], 0.25)]
    xfree_nodes, ufree_nodes = x_src >= 0, u_src >= 0
    t = lambda a, dt=F64: torch.as_tensor(a, dtype=dt).to(DEV).contiguous()
    full = lambda shape, v=SENTINEL: torch.full(shape, v, dtype=F64, device=DEV)
    st = stream_ptr(DEV)
    w = 0.7
    for suffix, dt in (("", F64), ("_f32", torch.float32)):
        fn = lambda name: getattr(L, f"hfem_{kind}_{name}{suffix}")
        cast = lambda a: t(a, dt).double().cpu().numpy()                  # what the kernel sees of fp32 rows
        Xk, Uk = np.empty_like(X), np.empty_like(U)
        Xk[xfree_nodes], Xk[~xfree_nodes] = cast(x_free)[x_src[xfree_nodes]], cast(x_fixed)[-1 - x_src[~xfree_nodes]]
        Uk[ufree_nodes], Uk[~ufree_nodes] = cast(u_free)[u_src[ufree_nodes]], cast(u_fixed)[-1 - u_src[~ufree_nodes]]
        Rk = cast(Xref)
        c32, s32, us32 = t(conn, torch.int32), t(x_src, torch.int32), t(u_src, torch.int32)
        xf, xx, xr, uf, ux = t(x_free, dt), t(x_fixed, dt), t(Xref, dt), t(u_free, dt), t(u_fixed, dt)
        lead = (0, ptr(c32), ne, ptr(s32), ptr(xf), ptr(xx))
        hyper = lead + (ptr(us32), ptr(uf), ptr(ux))
        n1 = max(ne, 1)
        q, r, j = full((n1,)), full((n1,)), full((n1,))
        summ, summ_null, jsum, jsum_null = full((3,)), full((3,)), full((2,)), full((2,))
        check(fn("mesh_measure")(*lead, ptr(xr), ptr(q), ptr(r), ptr(summ), st), "measure")
        check(fn("mesh_measure")(*lead, ptr(xr), None, None, ptr(summ_null), st), "measure, no per-element outputs")
        check(fn("deformation_measure")(*hyper, ptr(j), ptr(jsum), st), "deformation")
        check(fn("deformation_measure")(*hyper, None, ptr(jsum_null), st), "deformation, no per-element output")
        alpha, halpha = full((len(directions),)), full((len(directions),))
        for i, (_, dn, eta) in enumerate(directions):
            d = t(dn)
            check(fn("step_bound")(*lead, ptr(d), eta, alpha.data_ptr() + 8 * i, st), "bound")
            check(fn("hyper_step_bound")(*hyper, ptr(d), eta, halpha.data_ptr() + 8 * i, st), "hyper bound")
        val, val_only = full((), 3.0), full((), 3.0)
        grad = full((x_free.shape[0], 2), 1.0)
        check(fn("quality_barrier")(*lead, ptr(xr), w, ptr(val), ptr(grad), st), "barrier")
        check(fn("quality_barrier")(*lead, ptr(xr), w, ptr(val_only), None, st), "barrier, value only")
        summ, summ_null, jsum, jsum_null = summ.tolist(), summ_null.tolist(), jsum.tolist(), jsum_null.tolist()
        if ne == 0:
            # nothing but the sentinels of the init launches: the keys of no element (NaN after the finish), the count 0
            assert math.isnan(summ[0]) and math.isnan(summ[1]) and summ[2] == 0.0 and math.isnan(jsum[0]) and jsum[1] == 0.0
            assert math.isnan(summ_null[0]) and math.isnan(summ_null[1]) and summ_null[2] == 0.0
            assert math.isnan(jsum_null[0]) and jsum_null[1] == 0.0
            assert (alpha == math.inf).all() and (halpha == math.inf).all()
            assert val.item() == 3.0 and val_only.item() == 3.0 and (grad == 1.0).all()
            assert (q == SENTINEL).all() and (r == SENTINEL).all() and (j == SENTINEL).all()
            continue
        wq, wr, winv, wj = _measures(kind, Xk, Rk, Uk, conn)
        assert not winv.any() and (wj > 0.0).all() and (wq > 0.0).all()          # the reference decides: a valid case
        gq, gr, gj = q.cpu().numpy(), r.cpu().numpy(), j.cpu().numpy()
        assert np.abs(gq - wq).max() <= 1e-13 * np.abs(wq).max()
        assert np.abs(gr - wr).max() <= 1e-13 * np.abs(wr).max()
        assert np.abs(gj - wj).max() <= 1e-13 * np.abs(wj).max()
        assert summ[0] == q.min().item() and summ[1] == r.min().item() and summ[2] == float(winv.sum()) == 0.0
        assert jsum[0] == j.min().item() and jsum[1] == 0.0
        assert summ_null == summ and jsum_null == jsum                    # the optional outputs change nothing else
        for i, (what, dn, eta) in enumerate(directions):
            D = np.zeros_like(X)
            D[xfree_nodes] = dn[x_src[xfree_nodes]]
            wa, wha = _bounds(kind, Xk, Uk, D, conn, eta)
            got, hgot = alpha[i].item(), halpha[i].item()
            if ne == 1 and what == "along u" and math.isinf(wha):         # a single element may only grow along its own u
                assert wa == got == hgot == math.inf
                continue
            assert math.isfinite(wa) and abs(got - wa) <= 1e-12 * wa, (what, eta)
            assert math.isfinite(wha) and abs(hgot - wha) <= 1e-12 * wha, (what, eta)
            assert hgot <= got                                            # the reference crossing is one of the two
            if ne > 1 and what == "along u":
                assert wha < wa                                           # ... and here the det F crossing is the active one
        wv, wg = barrier_torch(torch.as_tensor(Xk), torch.as_tensor(Rk), torch.as_tensor(conn).long(),
                               torch.as_tensor(np.nonzero(xfree_nodes)[0]), w)
        got_g = np.zeros_like(X)
        got_g[xfree_nodes] = (grad.cpu().numpy() - 1.0)[x_src[xfree_nodes]]     # ACCUMULATED onto the ones
        assert abs(val.item() - 3.0 - wv) <= 1e-11 * abs(wv) and abs(val_only.item() - 3.0 - wv) <= 1e-11 * abs(wv)
        assert np.abs(got_g[xfree_nodes] - wg.numpy()).max() <= 1e-11 * wg.abs().max().item()
