"""The QUAD4 r-adaptive solve's host surface, without a GPU: the six mesh-validity entry points are exported and bound, argument
errors come back as negative codes with a message before any device is touched, the Python API refuses what it does not
support and dispatches on the element kind, and the numpy closed forms of the corner cross products, the measure and the step
bound (the oracles tests/test_gpu_radapt_quad4.py checks the kernels against) agree with a brute-force scan of the four
c_k(alpha) and with hand-worked cases."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

QUAD4_MESH_SYMBOLS = ["hfem_quad4_mesh_measure", "hfem_quad4_step_bound", "hfem_quad4_quality_barrier"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def test_quad4_mesh_symbols_are_exported_and_bound_and_the_version_is_unchanged():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    for n in QUAD4_MESH_SYMBOLS + [s + "_f32" for s in QUAD4_MESH_SYMBOLS]:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
        assert L.PROTOTYPES[n] == L.PROTOTYPES[n.replace("quad4", "tri3")], n       # the TRI3 argument lists exactly
    assert L.lib().hfem_version() == 114


def test_quad4_mesh_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    buf = (C.c_double * 8)()
    conn = (C.c_int32 * 4)(0, 1, 2, 3)
    xs = (C.c_int32 * 4)(0, 1, 2, 3)
    p = C.addressof(buf)
    for suffix in ("", "_f32"):
        measure = getattr(lib, "hfem_quad4_mesh_measure" + suffix)
        bound = getattr(lib, "hfem_quad4_step_bound" + suffix)
        barrier = getattr(lib, "hfem_quad4_quality_barrier" + suffix)
        assert measure(0, conn, 1, xs, p, None, p, None, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert measure(0, conn, -1, xs, p, None, p, None, None, p, None) < 0 and b"ne must be" in lib.hfem_last_error()
        assert measure(0, conn, 1 << 31, xs, p, None, p, None, None, p, None) < 0 and b"ne must be" in lib.hfem_last_error()
        assert measure(0, None, 1, xs, p, None, p, None, None, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert measure(0, conn, 1, xs, p, None, None, None, None, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert bound(0, conn, 1, xs, p, None, None, 0.25, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert bound(0, conn, -5, xs, p, None, p, 0.25, p, None) < 0 and b"ne must be" in lib.hfem_last_error()
        for eta in (0.0, 1.0, -0.5, 1.5, math.nan):
            assert bound(0, conn, 1, xs, p, None, p, eta, p, None) < 0 and b"eta must be in (0, 1)" in lib.hfem_last_error()
        assert barrier(0, conn, 1, xs, p, None, p, 1.0, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert barrier(0, conn, -1, xs, p, None, p, 1.0, p, None, None) < 0 and b"ne must be" in lib.hfem_last_error()
        for w in (-1.0, math.inf, math.nan):
            assert barrier(0, conn, 1, xs, p, None, p, w, p, None, None) < 0 and b"weight" in lib.hfem_last_error()
        assert bound(0, None, 1, xs, p, None, p, 0.25, p, None) < 0 and b"quad4_step_bound" in lib.hfem_last_error()


def _model(quad=True):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    if quad:
        nc, conn, geom, bc, mn, edges = structured_quad_mesh(7, 5, dtype=torch.float64)
        return QuadShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(7, 5, dtype=torch.float64)
    return PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)


def test_quad4_python_api_refuses_tri3_deterministic_and_planless_losses_and_a_bad_eta():
    from hidenn_fem_amd import radapt
    from hidenn_fem_amd.loss import EnergyLoss2D
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    quad, tri = _model(), _model(quad=False)
    with pytest.raises(NotImplementedError, match="QUAD4 models only"):
        radapt.Quad4RAdaptiveSolver(tri, lf)
    for fn in (radapt.quad4_mesh_quality, lambda m: radapt.quad4_max_feasible_step(m, torch.zeros_like(m.node_coords_free)),
               radapt.quad4_quality_barrier):
        with pytest.raises(NotImplementedError, match="QUAD4 models only"):
            fn(tri)
    # the TRI3 side still refuses QUAD4, and now says where to go
    with pytest.raises(NotImplementedError, match="TRI3 models only.*Quad4RAdaptiveSolver"):
        radapt.RAdaptiveSolver(quad, lf)
    with pytest.raises(NotImplementedError, match="TRI3 models only.*quad4_mesh_quality"):
        radapt.mesh_quality(quad)
    with pytest.raises(NotImplementedError, match="deterministic"):
        radapt.Quad4RAdaptiveSolver(quad, EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True))
    planless = EnergyLoss2D(device=cpu, dtype=torch.float64)
    planless.quad4_planless = True
    with pytest.raises(NotImplementedError, match="quad4_planless"):
        radapt.Quad4RAdaptiveSolver(quad, planless)
    for eta in (0.0, 1.0, -0.1, 2.0):
        with pytest.raises(ValueError, match="eta"):
            radapt.Quad4RAdaptiveSolver(quad, lf, eta=eta)
        with pytest.raises(ValueError, match="eta"):
            radapt.quad4_max_feasible_step(quad, torch.zeros_like(quad.node_coords_free), eta=eta)
    with pytest.raises(ValueError):
        radapt.Quad4RAdaptiveSolver(quad, lf, history=-1)
    with pytest.raises(ValueError):
        radapt.Quad4RAdaptiveSolver(quad, lf, quality_weight=-1.0)
    if not torch.cuda.is_available():
        for fn in (radapt.quad4_mesh_quality, lambda m: radapt.Quad4RAdaptiveSolver(m, lf), lambda m: radapt.r_adapt_(m, lf)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(quad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            radapt.r_adapt_(tri, lf)


def test_r_adapt_picks_the_class_by_element_kind(monkeypatch):
    from hidenn_fem_amd import radapt
    made = []

    def fake(name):
        class Fake:
            def __init__(self, model, loss_fn, **kw):
                made.append((name, model, loss_fn, kw))

            def run(self):
                return name + ".run"
        return Fake

    monkeypatch.setattr(radapt, "RAdaptiveSolver", fake("tri3"))
    monkeypatch.setattr(radapt, "Quad4RAdaptiveSolver", fake("quad4"))
    quad, tri, lf = _model(), _model(quad=False), object()
    assert radapt.r_adapt_(quad, lf, max_outer=3, eta=0.5) == "quad4.run"
    assert radapt.r_adapt_(tri, lf) == "tri3.run"
    assert made == [("quad4", quad, lf, dict(max_outer=3, eta=0.5)), ("tri3", tri, lf, {})]


def test_the_two_solver_classes_share_one_loop():
    from hidenn_fem_amd import radapt
    for name in ("run", "_line_search", "_direction", "objective", "objective_and_grad", "solve_and_grad", "__init__"):
        assert getattr(radapt.RAdaptiveSolver, name) is getattr(radapt.Quad4RAdaptiveSolver, name), name


# ---------------------------------------------------------------- the numpy oracles
def quad4_corners_np(X):
    """c [Ne, 4] and S [Ne, 4] of corner rows X [Ne, 4, 2]: c_k = (X_k+1 - X_k) x (X_k-1 - X_k), S_k = the two squared lengths."""
    a = np.roll(X, -1, axis=1) - X
    b = np.roll(X, 1, axis=1) - X
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0], (a ** 2).sum(axis=-1) + (b ** 2).sum(axis=-1)


def quad4_measure_np(X, Xref):
    """(q [Ne], det_ratio [Ne], inverted [Ne] bool) of corner rows X against the reference rows Xref (both [Ne, 4, 2])."""
    c, S = quad4_corners_np(X)
    cr, _ = quad4_corners_np(Xref)
    s = np.sign(cr[:, 0] + cr[:, 2])[:, None]
    return (2.0 * s * c / S).min(axis=1), (c / cr).min(axis=1), (s * c <= 0.0).any(axis=1)


def quad4_step_bound_np(X, D, eta):
    """Per element: the smallest alpha > 0 at which some corner has c_k(X + alpha D) = eta c_k(X) (inf if none; 0 if some
    c_k(X) = 0).  X, D: [Ne, 4, 2] corner rows.  Returns (bound [Ne], A0, A1, A2 [Ne, 4]) with c_k(alpha) = A0 + A1 alpha +
    A2 alpha^2.  The closed form of csrc/hfem_crossing_dev.h first_crossing, written independently over arrays."""
    a, b = np.roll(X, -1, axis=1) - X, np.roll(X, 1, axis=1) - X
    da, db = np.roll(D, -1, axis=1) - D, np.roll(D, 1, axis=1) - D
    cr = lambda p, r: p[..., 0] * r[..., 1] - p[..., 1] * r[..., 0]
    A0, A1, A2 = cr(a, b), cr(a, db) + cr(da, b), cr(da, db)
    sg = np.where(A0 > 0.0, 1.0, -1.0)
    c, bb, aa = (1.0 - eta) * A0 * sg, A1 * sg, A2 * sg
    disc = bb * bb - 4.0 * aa * c
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.where(disc >= 0.0, disc, 0.0))
        root_b = c / (0.5 * (sq - bb))                      # b < 0: the smaller positive root (the linear case for a2 = 0)
        root_a = (-0.5 * (bb + sq)) / aa                    # b >= 0, a2 < 0: the positive root
    out = np.full(A0.shape, np.inf)
    out = np.where((disc >= 0.0) & (bb >= 0.0) & (aa < 0.0), root_a, out)
    out = np.where((disc >= 0.0) & (bb < 0.0), root_b, out)
    out = np.where(A0 == 0.0, 0.0, out)
    return out.min(axis=1), A0, A1, A2


def _jittered_unit_cells(n, rng):
    """Unit squares with uniform jitter +-0.2 per coordinate: every corner cross product stays >= 0.2, so every cell is convex
    (the edge vectors at a corner are (1 + u, v) and (w, 1 + z) with |u|, |v|, |w|, |z| <= 0.4: c >= 0.6^2 - 0.4^2 = 0.2)."""
    base = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    return base[None] + rng.uniform(-0.2, 0.2, size=(n, 4, 2))


def _scan4(A0, A1, A2, eta, amax=20.0, n=200001):
    """First alpha on a fine grid where some corner's sign(A0) (c_k(alpha) - eta c_k(0)) reaches 0, refined by bisection (inf if
    none up to amax).  A0, A1, A2: [4]."""
    f = lambda t: ((A0 + A1 * t + A2 * t * t - eta * A0) * np.sign(A0)).min()
    al = np.linspace(0.0, amax, n)
    v = ((A0[:, None] + A1[:, None] * al + A2[:, None] * al * al - eta * A0[:, None]) * np.sign(A0)[:, None]).min(axis=0)
    hit = np.nonzero(v[1:] <= 0.0)[0]
    if hit.size == 0:
        return np.inf
    lo, hi = al[hit[0]], al[hit[0] + 1]
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0.0 else (lo, mid)
    return hi


def test_numpy_quad4_step_bound_agrees_with_a_brute_force_scan_on_random_jittered_cells():
    rng = np.random.default_rng(0)
    n = 300
    X = _jittered_unit_cells(n, rng)
    c, _ = quad4_corners_np(X)
    assert c.min() >= 0.2
    D = rng.normal(size=(n, 4, 2)) * 10.0 ** rng.uniform(-3.0, 0.3, size=(n, 1, 1))
    eta = 0.25
    got, A0, A1, A2 = quad4_step_bound_np(X, D, eta)
    assert np.array_equal(A0, c)
    kinds = set()
    for i in range(n):
        want = _scan4(A0[i], A1[i], A2[i], eta)
        if np.isinf(want):
            kinds.add("none")
            assert np.isinf(got[i]) or got[i] > 20.0, (i, got[i])
        else:
            kinds.add("root")
            assert abs(got[i] - want) <= 1e-9 * max(1.0, want), (i, got[i], want)
    assert kinds == {"none", "root"}


def test_corner_values_bound_detj_at_the_gauss_points():
    """detJ(xi, eta) of a bilinear cell is the bilinear interpolant of c_k / 4, so a step that keeps a share of every c_k keeps
    at least that share of detJ at the 2x2 Gauss points."""
    rng = np.random.default_rng(1)
    X = _jittered_unit_cells(200, rng)
    D = rng.normal(size=X.shape)
    xi_k, eta_k = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    g = 1.0 / math.sqrt(3.0)

    def detj(P, xi, et):
        d0, d1 = 0.25 * xi_k * (1.0 + eta_k * et), 0.25 * eta_k * (1.0 + xi_k * xi)
        J = np.einsum("k,ekc->ec", d0, P), np.einsum("k,ekc->ec", d1, P)
        return J[0][:, 0] * J[1][:, 1] - J[0][:, 1] * J[1][:, 0]

    c, _ = quad4_corners_np(X)
    for k in range(4):
        assert np.abs(detj(X, xi_k[k], eta_k[k]) - 0.25 * c[:, k]).max() <= 1e-15
    for eta in (0.25, 0.6):
        a, *_ = quad4_step_bound_np(X, D, eta)
        ok = np.isfinite(a)                                     # a few directions have no crossing at all
        assert ok.sum() >= 150
        X1, Y = X[ok], X[ok] + a[ok, None, None] * D[ok]
        cy, _ = quad4_corners_np(Y)
        assert np.abs((cy / c[ok]).min(axis=1) - eta).max() <= 1e-11
        for xi in (-g, g):
            for et in (-g, g):
                assert (detj(Y, xi, et) / detj(X1, xi, et)).min() >= eta


def test_numpy_quad4_step_bound_closed_cases():
    eta = 0.25
    X = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]])
    q, r, inv = quad4_measure_np(X, X)
    assert q[0] == 1.0 and r[0] == 1.0 and not inv[0]
    qcw, rcw, invcw = quad4_measure_np(X[:, ::-1], X[:, ::-1])      # clockwise numbering: s = -1, the same measure
    assert qcw[0] == 1.0 and rcw[0] == 1.0 and not invcw[0]
    # d = 0 everywhere, and a rigid translation: no crossing
    got, *_ = quad4_step_bound_np(X, np.zeros_like(X), eta)
    assert np.isinf(got[0])
    got, *_ = quad4_step_bound_np(X, np.broadcast_to([0.3, -0.7], X.shape).copy(), eta)
    assert np.isinf(got[0])
    # uniform shrinking toward the origin, d = -X: every c_k(alpha) = (1 - alpha)^2 c_k, first crossing at 1 - sqrt(eta)
    got, *_ = quad4_step_bound_np(X, -X, eta)
    assert abs(got[0] - (1.0 - math.sqrt(eta))) <= 1e-15
    # corner 2 = (1, 1) pushed straight at the opposite diagonal (through corners 1 and 3), reaching it at alpha = 1: every
    # c_k is linear in alpha (one node moves); c_2 = 1 - alpha, c_1 = c_3 = 1 - alpha / 2, c_0 = 1: the bound is 1 - eta
    D = np.zeros_like(X)
    D[0, 2] = [-0.5, -0.5]
    got, A0, A1, A2 = quad4_step_bound_np(X, D, eta)
    assert (A2[0] == 0.0).all() and (A0[0] == 1.0).all() and list(A1[0]) == [0.0, -0.5, -1.0, -0.5]
    assert abs(got[0] - (1.0 - eta)) <= 1e-15
    assert abs(_scan4(A0[0], A1[0], A2[0], eta) - got[0]) <= 1e-9
    _, r, inv = quad4_measure_np(X + 1.0 * D, X)
    assert r[0] == 0.0 and inv[0]                                   # on the diagonal: corner 2 is flat
    # moving away from the diagonal: never crosses
    got, *_ = quad4_step_bound_np(X, -D, eta)
    assert np.isinf(got[0])
    # three collinear corners (0, 1, 2): c_1 = 0, no share of nothing can be kept
    got, A0, *_ = quad4_step_bound_np(np.array([[[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [0.0, 1.0]]]), np.ones((1, 4, 2)), eta)
    assert A0[0, 1] == 0.0 and got[0] == 0.0
