"""The finite-strain r-adaptive solve's host surface, without a GPU: the numpy closed forms of the det F-safe step bound (the
oracles tests/test_gpu_hyper_radapt.py checks the kernels against) agree with a brute-force scan of det F(alpha) - eta det F(0)
and of R(alpha) - eta R(0); the QUAD4 bound guarantees what DESIGN 22 says it does; the eight entry points are exported, bound
and prototyped; argument errors come back as negative codes with a message before any device is touched; the Python API
refuses what it does not support and dispatches on the loss; and csrc/hfem_mesh_elem_dev.h runs clean under the address and
undefined-behaviour sanitizers as a stand-alone host program."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from test_radapt_host import _measure_np, step_bound_np
from test_radapt_quad4_host import _jittered_unit_cells, quad4_corners_np, quad4_measure_np

HYPER_MESH_SYMBOLS = ["hfem_tri3_hyper_step_bound", "hfem_tri3_deformation_measure", "hfem_quad4_hyper_step_bound",
                      "hfem_quad4_deformation_measure"]


# ---------------------------------------------------------------- the numpy oracles
def first_positive_root(c0, c1, c2):
    """The smallest a > 0 with c0 + c1 a + c2 a^2 = 0 for c0 > 0 (inf if none), by the textbook stable pair of roots
    q / c2 and c0 / q with q = -(c1 + sign(c1) sqrt(disc)) / 2 -- not the branch structure of csrc/hfem_crossing_dev.h."""
    if c2 == 0.0:
        return -c0 / c1 if c1 < 0.0 else math.inf
    disc = c1 * c1 - 4.0 * c2 * c0
    if disc < 0.0:
        return math.inf
    q = -0.5 * (c1 + math.copysign(math.sqrt(disc), c1))
    pos = [r for r in (q / c2, c0 / q) if r > 0.0]
    return min(pos) if pos else math.inf


def crossings_np(A, B, eta):
    """(reference crossing, det F crossing) of ONE pair of quadratics R = A[0] + A[1] a + A[2] a^2, D = B[0] + ...: the first
    a > 0 with R(a) = eta R(0), and the first with D(a) R(0) = eta D(0) R(a) (0 when R(0) D(0) <= 0 or NaN)."""
    A0, A1, A2 = (float(v) for v in A)
    B0, B1, B2 = (float(v) for v in B)
    if A0 == 0.0:
        ref = 0.0
    else:
        sg = 1.0 if A0 > 0.0 else -1.0
        ref = first_positive_root((1.0 - eta) * A0 * sg, A1 * sg, A2 * sg)
    if not A0 * B0 > 0.0:
        return ref, 0.0
    return ref, first_positive_root((1.0 - eta) * A0 * B0, B1 * A0 - eta * B0 * A1, B2 * A0 - eta * B0 * A2)


def hyper_step_bound_np(X, U, D, eta):
    """TRI3, per element: (bound, reference crossing, det F crossing, A [Ne, 3], B [Ne, 3]) for corner rows X, displacement rows
    U and direction rows D, all [Ne, 3, 2]; R(a) = detJ(X + a D), D(a) = detJ(X + U + a D)."""
    A = np.stack(step_bound_np(X, D, eta)[1:], axis=1)
    B = np.stack(step_bound_np(X + U, D, eta)[1:], axis=1)
    cr = np.array([crossings_np(A[i], B[i], eta) for i in range(A.shape[0])]).reshape(-1, 2)
    return np.fmin(cr[:, 0], cr[:, 1]), cr[:, 0], cr[:, 1], A, B


def quad4_coefficients_np(X, D):
    """[Ne, 4, 3]: c_k(X + a D) = A0 + A1 a + A2 a^2 per corner, c_k = (X_k+1 - X_k) x (X_k-1 - X_k)."""
    a, b = np.roll(X, -1, axis=1) - X, np.roll(X, 1, axis=1) - X
    da, db = np.roll(D, -1, axis=1) - D, np.roll(D, 1, axis=1) - D
    cr = lambda p, r: p[..., 0] * r[..., 1] - p[..., 1] * r[..., 0]
    return np.stack([cr(a, b), cr(a, db) + cr(da, b), cr(da, db)], axis=-1)


def quad4_hyper_step_bound_np(X, U, D, eta):
    """QUAD4, per cell: (bound, reference crossing, det F crossing, A [Ne, 4, 3], B [Ne, 4, 3]), each crossing the minimum over
    the four corners of the corner-wise one."""
    A, B = quad4_coefficients_np(X, D), quad4_coefficients_np(X + U, D)
    cr = np.array([[crossings_np(A[i, k], B[i, k], eta) for k in range(4)] for i in range(A.shape[0])]).reshape(-1, 4, 2)
    ref, dfc = cr[..., 0].min(axis=1), cr[..., 1].min(axis=1)
    return np.fmin(ref, dfc), ref, dfc, A, B


def det_f_np(X, U):
    """TRI3 det F [Ne] = detJ(X + U) / detJ(X)."""
    det = lambda T: (T[:, 0, 0] - T[:, 2, 0]) * (T[:, 1, 1] - T[:, 2, 1]) - (T[:, 1, 0] - T[:, 2, 0]) * (T[:, 0, 1] - T[:, 2, 1])
    return det(X + U) / det(X)


def quad4_corner_ratios_np(X, U):
    """r [Ne, 4] = c_k^def / c_k; a cell's J is r.min(axis=1)."""
    return quad4_corners_np(X + U)[0] / quad4_corners_np(X)[0]


def barrier_terms_torch(P, R, weight):
    """[Ne] tensor: an element's share of Q = (w / (terms Ne)) sum (1/q - 1) (TRI3: terms = 1, q = 2 sqrt(3) s detJ / sum |e|^2;
    QUAD4: terms = 4, the sum runs over the corners, q_k = 2 s c_k / (|e_k-1|^2 + |e_k|^2)), as hidenn_fem_amd/radapt.py states
    it.  P, R: [Ne, 3 or 4, 2] fp64 tensors, the current and the reference corner rows; differentiable in P."""
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    ne, npe = P.shape[0], P.shape[1]
    if npe == 3:
        det = lambda T: cross(T[:, 0] - T[:, 2], T[:, 1] - T[:, 2])
        S = sum(((P[:, (i + 1) % 3] - P[:, i]) ** 2).sum(dim=1) for i in range(3))
        q = 2.0 * math.sqrt(3.0) * torch.sign(det(R)) * det(P) / S
        return weight / ne * (1.0 / q - 1.0)

    def corners(T):
        a, b = torch.roll(T, -1, dims=1) - T, torch.roll(T, 1, dims=1) - T
        return cross(a, b), (a ** 2).sum(dim=-1) + (b ** 2).sum(dim=-1)

    c, S = corners(P)
    cr, _ = corners(R)
    q = 2.0 * torch.sign(cr[:, 0] + cr[:, 2])[:, None] * c / S
    return weight / (4.0 * ne) * (1.0 / q - 1.0).sum(dim=1)


def barrier_torch(X, Xr, conn, idx_free, weight):
    """(Q, dQ/d(rows idx_free of X)) by autograd on the CPU; X, Xr [Nn, 2] fp64 tensors, conn [Ne, 3 or 4] long."""
    xf = X[idx_free].clone().requires_grad_(True)
    full = X.clone()
    full[idx_free] = xf
    Q = barrier_terms_torch(full[conn], Xr[conn], weight).sum()
    (g,) = torch.autograd.grad(Q, xf)
    return Q.item(), g


def kind_of(ref, dfc):
    return "none" if math.isinf(ref) and math.isinf(dfc) else ("reference" if ref <= dfc else "det_f")


# ---------------------------------------------------------------- brute force
def _scan_hyper(A, B, eta, amax, n):
    """A, B: [m, 3] (m = 1: a triangle; 4: the corners of a cell), valid at 0.  The first alpha on a fine grid, refined by
    bisection, at which some row's R(alpha) - eta R(0) or det F(alpha) - eta det F(0) reaches 0 -> (alpha or inf, kind)."""
    A, B = np.asarray(A, dtype=float).reshape(-1, 3), np.asarray(B, dtype=float).reshape(-1, 3)
    sg = np.sign(A[:, 0])[:, None]

    def f(t):                                               # [2, len(t)]: both > 0 before the first crossing
        t = np.atleast_1d(np.asarray(t, dtype=float))[None, :]
        R = A[:, 0:1] + A[:, 1:2] * t + A[:, 2:3] * t * t
        Dd = B[:, 0:1] + B[:, 1:2] * t + B[:, 2:3] * t * t
        fr = (R - eta * A[:, 0:1]) / A[:, 0:1]
        with np.errstate(divide="ignore", invalid="ignore"):
            fd = (Dd / R) / (B[:, 0:1] / A[:, 0:1]) - eta
        fd = np.where(R * sg > 0.0, fd, -1.0)               # past R = 0 the reference crossing has long been met
        return np.stack([fr.min(axis=0), fd.min(axis=0)])

    al = np.linspace(0.0, amax, n)
    v = f(al).min(axis=0)
    hit = np.nonzero(v[1:] <= 0.0)[0]
    if hit.size == 0:
        return math.inf, "none"
    lo, hi = al[hit[0]], al[hit[0] + 1]
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid).min() > 0.0 else (lo, mid)
    fr, fd = f(hi)[:, 0]
    return hi, ("reference" if fr <= fd else "det_f")


def _valid(rows, corners, floor=0.0):
    """Indices of the elements whose deformed state is valid: every det / corner cross product of X and of X + U above `floor`."""
    return np.nonzero((corners > floor).reshape(rows, -1).all(axis=1))[0]


def _random_triangles(n, rng):
    """n random counter-clockwise triangles with a valid deformed state, and directions of mixed size."""
    X = rng.normal(size=(4 * n, 3, 2))
    U = rng.normal(size=X.shape) * rng.uniform(0.02, 0.5, size=(4 * n, 1, 1))
    det = lambda T: (T[:, 0, 0] - T[:, 2, 0]) * (T[:, 1, 1] - T[:, 2, 1]) - (T[:, 1, 0] - T[:, 2, 0]) * (T[:, 0, 1] - T[:, 2, 1])
    keep = _valid(4 * n, np.stack([det(X), det(X + U)], axis=1))[:n]
    assert keep.size == n
    D = rng.normal(size=(n, 3, 2)) * rng.uniform(0.05, 2.0, size=(n, 1, 1))
    return X[keep], U[keep], D


def _random_cells(n, rng, scale=(-3.0, 0.3)):
    """n jittered unit cells (every c_k >= 0.2) with displacement rows that leave every deformed corner convex, c_k^def >=
    0.05: the corner ratios are then no smaller than 0.05 / 1.96 and dividing by them costs two digits at the most."""
    X = _jittered_unit_cells(4 * n, rng)
    U = rng.uniform(-1.0, 1.0, size=X.shape) * rng.uniform(0.02, 0.4, size=(4 * n, 1, 1))
    keep = _valid(4 * n, quad4_corners_np(X + U)[0], floor=0.05)[:n]
    assert keep.size == n
    D = rng.normal(size=(n, 4, 2)) * 10.0 ** rng.uniform(*scale, size=(n, 1, 1))
    return X[keep], U[keep], D


def test_numpy_hyper_step_bound_agrees_with_a_brute_force_scan_on_random_triangles():
    rng = np.random.default_rng(0)
    n, eta = 300, 0.25
    X, U, D = _random_triangles(n, rng)
    assert (det_f_np(X, U) > 0.0).all()
    got, ref, dfc, A, B = hyper_step_bound_np(X, U, D, eta)
    assert np.array_equal(A[:, 2], B[:, 2])                          # the same d moves both elements: B2 = A2
    kinds = set()
    for i in range(n):
        want, kind = _scan_hyper(A[i], B[i], eta, 50.0, 400001)
        kinds.add("none" if math.isinf(want) else kind_of(ref[i], dfc[i]))
        if math.isinf(want):
            assert np.isinf(got[i]) or got[i] > 50.0, (i, got[i])
        else:
            assert abs(got[i] - want) <= 1e-9 * max(1.0, want), (i, got[i], want, kind)
            if abs(ref[i] - dfc[i]) > 1e-6 * max(1.0, want):
                assert kind == kind_of(ref[i], dfc[i]), (i, kind, ref[i], dfc[i])
    assert kinds == {"reference", "det_f", "none"}


def test_numpy_quad4_hyper_step_bound_agrees_with_a_brute_force_scan_on_random_cells():
    rng = np.random.default_rng(0)
    n, eta = 300, 0.25
    X, U, D = _random_cells(n, rng)
    got, ref, dfc, A, B = quad4_hyper_step_bound_np(X, U, D, eta)
    assert np.array_equal(A[..., 0], quad4_corners_np(X)[0]) and np.array_equal(A[..., 2], B[..., 2])
    kinds = set()
    for i in range(n):
        want, kind = _scan_hyper(A[i], B[i], eta, 20.0, 200001)
        kinds.add("none" if math.isinf(want) else kind_of(ref[i], dfc[i]))
        if math.isinf(want):
            assert np.isinf(got[i]) or got[i] > 20.0, (i, got[i])
        else:
            assert abs(got[i] - want) <= 1e-9 * max(1.0, want), (i, got[i], want, kind)
            if abs(ref[i] - dfc[i]) > 1e-6 * max(1.0, want):
                assert kind == kind_of(ref[i], dfc[i]), (i, kind, ref[i], dfc[i])
    assert kinds == {"reference", "det_f", "none"}


def test_numpy_hyper_step_bound_closed_cases():
    eta = 0.25
    X = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])
    zero = np.zeros_like(X)
    # u = 0: det F = 1 whatever the step, the det F polynomial is (1 - eta) R(0) R(a) and reaches 0 only where R does -- after
    # the reference crossing: the bound is the small-strain one, to the bit
    D = zero.copy()
    D[0, 2] = [0.5, -1.0]
    got, ref, dfc, *_ = hyper_step_bound_np(X, zero, D, eta)
    assert got[0] == ref[0] == step_bound_np(X, D, eta)[0][0] == 1.0 - eta and dfc[0] == 1.0
    # a zero direction: neither crossing
    got, ref, dfc, *_ = hyper_step_bound_np(X, 0.1 * X, zero, eta)
    assert np.isinf(got[0]) and np.isinf(ref[0]) and np.isinf(dfc[0])
    # node 2 displaced to (0, 0.2) (det F = 0.2) and pulled UP, d_2 = (0, 1): R(a) = 1 + a grows, D(a) = 0.2 + a, det F(a) =
    # (0.2 + a) / (1 + a) grows: no crossing.  Pushed DOWN, d_2 = (0, -1): the reference element keeps eta until a = 0.75, but
    # det F(a) = (0.2 - a) / (1 - a) = 0.05 at a = 3/19: the det F crossing is the active one, long before
    U = zero.copy()
    U[0, 2] = [0.0, -0.8]
    D[0, 2] = [0.0, 1.0]
    assert np.isinf(hyper_step_bound_np(X, U, D, eta)[0][0])
    got, ref, dfc, *_ = hyper_step_bound_np(X, U, -D, eta)
    assert ref[0] == 0.75 and abs(dfc[0] - 3.0 / 19.0) <= 1e-15 and got[0] == dfc[0]
    assert abs(det_f_np(X + got[0] * -D, U)[0] - eta * 0.2) <= 1e-15
    # a step that keeps the reference area exactly (node 2 slides parallel to its opposite edge) and still collapses det F:
    # u_1 = (0, 0.5) slants the deformed edge 0-1, u_2 = (0, -0.4): D(a) = 0.6 - 0.5 a while R = 1, det F(a) = 0.15 at a = 0.9
    U = zero.copy()
    U[0, 1] = [0.0, 0.5]
    U[0, 2] = [0.0, -0.4]
    D[0, 2] = [1.0, 0.0]
    got, ref, dfc, A, B = hyper_step_bound_np(X, U, D, eta)
    assert list(A[0]) == [1.0, 0.0, 0.0] and np.isinf(ref[0])
    assert abs(B[0, 0] - 0.6) <= 1e-15 and B[0, 1] == -0.5 and abs(got[0] - 0.9) <= 1e-15
    # an inverted state: det F < 0 -> 0
    U = zero.copy()
    U[0, 2] = [0.0, -1.5]
    got, ref, dfc, *_ = hyper_step_bound_np(X, U, D, eta)
    assert det_f_np(X, U)[0] == -0.5 and dfc[0] == 0.0 and got[0] == 0.0


def test_quad4_bound_keeps_det_f_at_every_point_above_eta_times_the_smallest_corner_ratio():
    """detJ of a bilinear cell is affine over the reference square, so det F at a point is sum_k w_k c_k^def / sum_k w_k c_k =
    a mean of the corner ratios r_k with the positive weights w_k c_k.  Below the bound every corner keeps eta of c_k and of
    r_k: det F at the Gauss points and the corners stays >= eta min_k r_k(0).  At the bound one corner lands on eta."""
    rng = np.random.default_rng(1)
    X, U, D = _random_cells(300, rng, scale=(-1.0, 0.5))
    xi_k, eta_k = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    g = 1.0 / math.sqrt(3.0)

    def detj(P, xi, et):
        d0, d1 = 0.25 * xi_k * (1.0 + eta_k * et), 0.25 * eta_k * (1.0 + xi_k * xi)
        J = np.einsum("k,ekc->ec", d0, P), np.einsum("k,ekc->ec", d1, P)
        return J[0][:, 0] * J[1][:, 1] - J[0][:, 1] * J[1][:, 0]

    points = [(-g, -g), (g, -g), (g, g), (-g, g)] + list(zip(xi_k, eta_k))
    r0 = quad4_corner_ratios_np(X, U)
    c0 = quad4_corners_np(X)[0]
    for xi, et in points:                                             # det F at a point is between the corner ratios
        F0 = detj(X + U, xi, et) / detj(X, xi, et)
        assert (F0 >= r0.min(axis=1) * (1 - 1e-14)).all() and (F0 <= r0.max(axis=1) * (1 + 1e-14)).all()
    for eta in (0.25, 0.6):
        a, ref, dfc, *_ = quad4_hyper_step_bound_np(X, U, D, eta)
        ok = a <= 20.0              # a few directions have no crossing; a far one is lost in the rounding of X + a D itself
        assert ok.sum() >= 200 and (ref[ok] < dfc[ok]).any() and (dfc[ok] < ref[ok]).any()
        Xo, Uo, Do, ao = X[ok], U[ok], D[ok], a[ok]
        floor = eta * r0[ok].min(axis=1)
        for frac in (0.3, 0.9, 0.999999):
            Y = Xo + (frac * ao)[:, None, None] * Do
            assert (quad4_corners_np(Y)[0] / c0[ok] >= eta).all()
            assert (quad4_corner_ratios_np(Y, Uo) / r0[ok] >= eta).all()
            for xi, et in points:
                assert (detj(Y + Uo, xi, et) / detj(Y, xi, et) >= floor).all()
        Y = Xo + ao[:, None, None] * Do
        landed = np.minimum(quad4_corners_np(Y)[0] / c0[ok], quad4_corner_ratios_np(Y, Uo) / r0[ok]).min(axis=1)
        assert np.abs(landed - eta).max() <= 1e-11


# ---------------------------------------------------------------- the library's host surface
def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def test_hyper_mesh_symbols_are_exported_bound_and_prototyped_and_the_version_is_unchanged():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    for n in HYPER_MESH_SYMBOLS + [s + "_f32" for s in HYPER_MESH_SYMBOLS]:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
        assert L.PROTOTYPES[n] == L.PROTOTYPES[n.replace("quad4", "tri3")], n
    # the step bound's argument list with u_src, u_free, u_fixed after the coordinate rows
    small, hyper = L.PROTOTYPES["hfem_tri3_step_bound"][1], L.PROTOTYPES["hfem_tri3_hyper_step_bound"][1]
    assert hyper[:6] == small[:6] and hyper[9:] == small[6:] and len(hyper) == len(small) + 3
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hidenn_fem.h")).read()
    for n in HYPER_MESH_SYMBOLS:
        assert n + "(" in text and n + "_f32(" in text, n
    assert L.lib().hfem_version() == 114


def test_hyper_mesh_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    for kind, npe in (("tri3", 3), ("quad4", 4)):
        conn = (C.c_int32 * npe)(*range(npe))
        xs = (C.c_int32 * npe)(*range(npe))
        us = (C.c_int32 * npe)(*range(npe))
        for suffix in ("", "_f32"):
            bound = getattr(lib, f"hfem_{kind}_hyper_step_bound{suffix}")
            measure = getattr(lib, f"hfem_{kind}_deformation_measure{suffix}")
            err = lib.hfem_last_error
            # bound(device, conn, ne, x_src, x_free, x_fixed, u_src, u_free, u_fixed, d, eta, alpha_out, stream)
            assert bound(0, conn, 1, xs, p, None, us, p, None, None, 0.25, p, None) < 0 and b"null pointer" in err()
            assert bound(0, conn, 1, xs, p, None, us, p, None, p, 0.25, None, None) < 0 and b"null pointer" in err()
            assert bound(0, conn, 1, xs, None, None, us, p, None, p, 0.25, p, None) < 0 and b"null pointer" in err()
            assert bound(0, conn, 1, xs, p, None, us, None, None, p, 0.25, p, None) < 0 and b"null pointer" in err()
            assert bound(0, conn, 1, xs, p, None, None, p, None, p, 0.25, p, None) < 0 and b"null pointer" in err()
            assert bound(0, conn, 1, None, p, None, us, p, None, p, 0.25, p, None) < 0 and b"null pointer" in err()
            assert bound(0, None, 1, xs, p, None, us, p, None, p, 0.25, p, None) < 0 and b"hyper_step_bound" in err()
            assert bound(0, conn, -5, xs, p, None, us, p, None, p, 0.25, p, None) < 0 and b"ne must be" in err()
            assert bound(0, conn, 1 << 31, xs, p, None, us, p, None, p, 0.25, p, None) < 0 and b"ne must be" in err()
            for eta in (0.0, 1.0, -0.5, 1.5, math.nan):
                assert bound(0, conn, 1, xs, p, None, us, p, None, p, eta, p, None) < 0 and b"eta must be in (0, 1)" in err()
            # measure(device, conn, ne, x_src, x_free, x_fixed, u_src, u_free, u_fixed, j_out, summary_out, stream)
            assert measure(0, conn, 1, xs, p, None, us, p, None, None, None, None) < 0 and b"null pointer" in err()
            assert measure(0, conn, 1, xs, None, None, us, p, None, None, p, None) < 0 and b"null pointer" in err()
            assert measure(0, conn, 1, xs, p, None, us, None, None, None, p, None) < 0 and b"null pointer" in err()
            assert measure(0, conn, 1, xs, p, None, None, p, None, None, p, None) < 0 and b"null pointer" in err()
            assert measure(0, None, 1, xs, p, None, us, p, None, None, p, None) < 0 and b"deformation_measure" in err()
            assert measure(0, conn, -1, xs, p, None, us, p, None, None, p, None) < 0 and b"ne must be" in err()
            assert measure(0, conn, 1 << 31, xs, p, None, us, p, None, None, p, None) < 0 and b"ne must be" in err()


def _model(quad=False):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    mesh = structured_quad_mesh if quad else structured_tri_mesh
    nc, conn, geom, bc, mn, edges = mesh(7, 5, dtype=torch.float64)
    return PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)


def test_hyper_python_api_refuses_linear_losses_the_wrong_element_kind_and_a_bad_eta():
    from hidenn_fem_amd import radapt
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    cpu = dict(device=torch.device("cpu"), dtype=torch.float64)
    lin, neo, neo4 = EnergyLoss2D(**cpu), NeoHookeanLoss2D(**cpu), Quad4NeoHookeanLoss2D(**cpu)
    quad, tri = _model(quad=True), _model()
    # linear losses: the message names the small-strain class of the same element kind
    with pytest.raises(NotImplementedError, match=r"NeoHookeanLoss2D only.*\bRAdaptiveSolver"):
        radapt.HyperRAdaptiveSolver(tri, lin)
    with pytest.raises(NotImplementedError, match="Quad4NeoHookeanLoss2D only.*Quad4RAdaptiveSolver"):
        radapt.Quad4HyperRAdaptiveSolver(quad, lin)
    # the wrong element kind, by the model or by the loss: the message names the other class
    for model, lf in ((quad, neo4), (quad, neo), (tri, neo4)):
        with pytest.raises(NotImplementedError, match="TRI3 models under a NeoHookeanLoss2D only.*Quad4HyperRAdaptiveSolver"):
            radapt.HyperRAdaptiveSolver(model, lf)
    for model, lf in ((tri, neo), (tri, neo4), (quad, neo)):
        with pytest.raises(NotImplementedError, match=r"QUAD4 models under a Quad4NeoHookeanLoss2D only.*: HyperRAdaptiveSolver"):
            radapt.Quad4HyperRAdaptiveSolver(model, lf)
    for fn in (radapt.deformation_measure, lambda m: radapt.hyper_max_feasible_step(m, torch.zeros_like(m.node_coords_free))):
        with pytest.raises(NotImplementedError, match="TRI3 models only.*quad4_deformation_measure"):
            fn(quad)
    for fn in (radapt.quad4_deformation_measure,
               lambda m: radapt.quad4_hyper_max_feasible_step(m, torch.zeros_like(m.node_coords_free))):
        with pytest.raises(NotImplementedError, match="QUAD4 models only.*hyper_max_feasible_step"):
            fn(tri)
    # the small-strain classes keep refusing a Neo-Hookean loss, and say where to go
    with pytest.raises(NotImplementedError, match="small-strain.*HyperRAdaptiveSolver"):
        radapt.RAdaptiveSolver(tri, neo)
    with pytest.raises(NotImplementedError, match="small-strain.*Quad4HyperRAdaptiveSolver"):
        radapt.Quad4RAdaptiveSolver(quad, neo4)
    for eta in (0.0, 1.0, -0.1, 2.0):
        with pytest.raises(ValueError, match="eta"):
            radapt.HyperRAdaptiveSolver(tri, neo, eta=eta)
        with pytest.raises(ValueError, match="eta"):
            radapt.Quad4HyperRAdaptiveSolver(quad, neo4, eta=eta)
        with pytest.raises(ValueError, match="eta"):
            radapt.hyper_max_feasible_step(tri, torch.zeros_like(tri.node_coords_free), eta=eta)
        with pytest.raises(ValueError, match="eta"):
            radapt.quad4_hyper_max_feasible_step(quad, torch.zeros_like(quad.node_coords_free), eta=eta)
    with pytest.raises(ValueError):
        radapt.HyperRAdaptiveSolver(tri, neo, history=-1)
    with pytest.raises(ValueError):
        radapt.Quad4HyperRAdaptiveSolver(quad, neo4, quality_weight=-1.0)
    with pytest.raises(TypeError):
        radapt.HyperRAdaptiveSolver(tri, neo, cg_rtol=1e-10)             # no CG keywords: the solve is Newton's
    if not torch.cuda.is_available():
        for fn in (radapt.deformation_measure, lambda m: radapt.HyperRAdaptiveSolver(m, neo), lambda m: radapt.r_adapt_(m, neo)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(tri)
        for fn in (radapt.quad4_deformation_measure, lambda m: radapt.Quad4HyperRAdaptiveSolver(m, neo4),
                   lambda m: radapt.r_adapt_(m, neo4)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(quad)


def test_r_adapt_picks_the_finite_strain_classes_for_a_neo_hookean_loss(monkeypatch):
    from hidenn_fem_amd import radapt
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D, Quad4NeoHookeanLoss2D
    made = []

    def fake(name):
        class Fake:
            def __init__(self, model, loss_fn, **kw):
                made.append((name, model, loss_fn, kw))

            def run(self):
                return name + ".run"
        return Fake

    for name in ("RAdaptiveSolver", "Quad4RAdaptiveSolver", "HyperRAdaptiveSolver", "Quad4HyperRAdaptiveSolver"):
        monkeypatch.setattr(radapt, name, fake(name))
    cpu = dict(device=torch.device("cpu"), dtype=torch.float64)
    lin, neo, neo4 = EnergyLoss2D(**cpu), NeoHookeanLoss2D(**cpu), Quad4NeoHookeanLoss2D(**cpu)
    quad, tri = _model(quad=True), _model()
    assert radapt.r_adapt_(tri, neo, max_outer=3, precond="amg") == "HyperRAdaptiveSolver.run"
    assert radapt.r_adapt_(quad, neo4) == "Quad4HyperRAdaptiveSolver.run"
    assert radapt.r_adapt_(tri, lin) == "RAdaptiveSolver.run" and radapt.r_adapt_(quad, lin) == "Quad4RAdaptiveSolver.run"
    assert made[0] == ("HyperRAdaptiveSolver", tri, neo, dict(max_outer=3, precond="amg"))
    assert [m[0] for m in made] == ["HyperRAdaptiveSolver", "Quad4HyperRAdaptiveSolver", "RAdaptiveSolver", "Quad4RAdaptiveSolver"]


def test_the_finite_strain_classes_run_the_small_strain_loop():
    from hidenn_fem_amd import radapt
    for name in ("run", "_line_search", "_direction", "objective", "objective_and_grad"):
        for cls in (radapt.HyperRAdaptiveSolver, radapt.Quad4HyperRAdaptiveSolver):
            assert getattr(cls, name) is getattr(radapt.RAdaptiveSolver, name), (cls, name)
    for name in ("__init__", "solve_and_grad", "_trial_share", "_step_extra"):
        assert getattr(radapt.HyperRAdaptiveSolver, name) is getattr(radapt.Quad4HyperRAdaptiveSolver, name), name
        assert getattr(radapt.HyperRAdaptiveSolver, name) is not getattr(radapt.RAdaptiveSolver, name), name
    assert radapt._HyperMesh.measure_f32_trials and radapt._QuadHyperMesh.measure_f32_trials      # both element kinds
    assert issubclass(radapt.HyperRAdaptInfo, radapt.RAdaptInfo)


# ---------------------------------------------------------------- the closed forms under the sanitizers
def test_hyper_mesh_closed_forms_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hfem_mesh_elem_dev.h (the text the kernels compile) as plain C++ against the stub <hip/hip_runtime.h>, built with
    -fsanitize=address,undefined and run as a child process: both crossings and J of every element within 1e-12 of this
    module's numpy values -- random valid triangles and cells, plus an inverted element and a zero direction of each kind --
    and, at the rows X + U against the reference rows X, the measure (q, ratio within 1e-12, the inverted flag) against the
    numpy forms and each element's barrier term and per-node gradient against CPU autograd (1e-11; the program's header has the
    rule).  CPU only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "hyper_mesh_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(here, "host", "hip_stub"), "-I", os.path.join(here, "..", "hidenn_fem_amd", "csrc"),
           os.path.join(here, "host", "hyper_mesh_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(7)
    eta, weight = 0.3, 0.7
    X3, U3, D3 = _random_triangles(200, rng)
    X4, U4, D4 = _random_cells(200, rng)
    for X, U, D in ((X3, U3, D3), (X4, U4, D4)):
        D[0] = 0.0                                                   # a zero direction
        U[1, 0] = X[1, 1:].mean(axis=0) - X[1, 0] + 1.5 * (X[1, 1:].mean(axis=0) - X[1, 0])   # node 0 far through the others
    _, ref3, def3, *_ = hyper_step_bound_np(X3, U3, D3, eta)
    _, ref4, def4, *_ = quad4_hyper_step_bound_np(X4, U4, D4, eta)
    J3, J4 = det_f_np(X3, U3), quad4_corner_ratios_np(X4, U4).min(axis=1)
    assert np.isinf(ref3[0]) and np.isinf(def3[0]) and np.isinf(ref4[0]) and np.isinf(def4[0])
    assert J3[1] < 0.0 and def3[1] == 0.0 and J4[1] < 0.0 and def4[1] == 0.0
    assert (J3[2:] > 0.0).all() and (J4[2:] > 0.0).all()
    # the measure of the rows X + U against the rows X: each element its own three / four nodes
    n3, n4 = X3.shape[0], X4.shape[0]
    q3, r3 = _measure_np((X3 + U3).reshape(-1, 2), X3.reshape(-1, 2), np.arange(3 * n3).reshape(n3, 3))
    inv3 = ~(q3 > 0.0)                                               # s detJ(X + U) <= 0: q carries that sign
    q4, r4, inv4 = quad4_measure_np(X4 + U4, X4)
    assert inv3[1] and inv4[1] and not inv3[2:].any() and not inv4[2:].any()
    assert np.array_equal(inv3, J3 <= 0.0) and np.array_equal(r4, J4)
    barrier = []
    for X, U in ((X3, U3), (X4, U4)):
        P = torch.as_tensor(X + U).requires_grad_(True)
        terms = barrier_terms_torch(P, torch.as_tensor(X), weight)
        (G,) = torch.autograd.grad(terms.sum(), P)
        barrier.append((terms.detach().numpy(), G.numpy()))
    assert all(np.isfinite(Q).all() and np.isfinite(G).all() and (Q[2:] > 0.0).all() for Q, G in barrier)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<2q", n3, n4))
        f.write(struct.pack("<2d", eta, weight))
        for a in (X3, U3, D3, ref3, def3, J3, q3, r3, inv3, *barrier[0], X4, U4, D4, ref4, def4, J4, q4, r4, inv4, *barrier[1]):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    run = subprocess.run([exe, path], capture_output=True, text=True)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("ok") == 2
