"""The r-adaptive solve's host surface, without a GPU: the mesh-validity entry points are exported and bound, argument errors
come back as negative codes with a message before any device is touched, the Python API refuses what it does not support, and
the numpy closed form of the step bound (the oracle tests/test_gpu_radapt.py checks the kernel against) agrees with a
brute-force scan of detJ(alpha)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

MESH_SYMBOLS = ["hfem_tri3_mesh_measure", "hfem_tri3_step_bound", "hfem_tri3_quality_barrier"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def test_mesh_symbols_are_exported_and_bound_and_the_version_is_unchanged():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    for n in MESH_SYMBOLS + [s + "_f32" for s in MESH_SYMBOLS]:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
    assert L.lib().hfem_version() == 114


def test_mesh_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    buf = (C.c_double * 8)()
    conn = (C.c_int32 * 3)(0, 1, 2)
    xs = (C.c_int32 * 3)(0, 1, 2)
    p = C.addressof(buf)
    for suffix in ("", "_f32"):
        measure = getattr(lib, "hfem_tri3_mesh_measure" + suffix)
        bound = getattr(lib, "hfem_tri3_step_bound" + suffix)
        barrier = getattr(lib, "hfem_tri3_quality_barrier" + suffix)
        assert measure(0, conn, 1, xs, p, None, p, None, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert measure(0, conn, -1, xs, p, None, p, None, None, p, None) < 0 and b"ne must be" in lib.hfem_last_error()
        assert measure(0, None, 1, xs, p, None, p, None, None, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert bound(0, conn, 1, xs, p, None, None, 0.25, p, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert bound(0, conn, -5, xs, p, None, p, 0.25, p, None) < 0 and b"ne must be" in lib.hfem_last_error()
        for eta in (0.0, 1.0, -0.5, 1.5, math.nan):
            assert bound(0, conn, 1, xs, p, None, p, eta, p, None) < 0 and b"eta must be in (0, 1)" in lib.hfem_last_error()
        assert barrier(0, conn, 1, xs, p, None, p, 1.0, None, None, None) < 0 and b"null pointer" in lib.hfem_last_error()
        assert barrier(0, conn, -1, xs, p, None, p, 1.0, p, None, None) < 0 and b"ne must be" in lib.hfem_last_error()
        assert barrier(0, conn, 1, xs, p, None, p, -1.0, p, None, None) < 0 and b"weight" in lib.hfem_last_error()
        assert bound(0, None, 1, xs, p, None, p, 0.25, p, None) < 0 and b"step_bound" in lib.hfem_last_error()


def _tri_model(quad=False):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    if quad:
        nc, conn, geom, bc, mn, edges = structured_quad_mesh(7, 5, dtype=torch.float64)
        return QuadShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)
    nc, conn, geom, bc, mn, edges = structured_tri_mesh(7, 5, dtype=torch.float64)
    return PiecewiseLinearShapeNN2D(nc, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges)


def test_python_api_refuses_quad4_deterministic_losses_and_a_bad_eta():
    from hidenn_fem_amd import radapt
    from hidenn_fem_amd.loss import EnergyLoss2D
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    quad, tri = _tri_model(quad=True), _tri_model()
    with pytest.raises(NotImplementedError, match="TRI3"):
        radapt.RAdaptiveSolver(quad, lf)
    for fn in (radapt.mesh_quality, lambda m: radapt.max_feasible_step(m, torch.zeros_like(m.node_coords_free)),
               radapt.quality_barrier):
        with pytest.raises(NotImplementedError, match="TRI3"):
            fn(quad)
    with pytest.raises(NotImplementedError, match="deterministic"):
        radapt.RAdaptiveSolver(tri, EnergyLoss2D(device=cpu, dtype=torch.float64, deterministic=True))
    for eta in (0.0, 1.0, -0.1, 2.0):
        with pytest.raises(ValueError, match="eta"):
            radapt.RAdaptiveSolver(tri, lf, eta=eta)
        with pytest.raises(ValueError, match="eta"):
            radapt.max_feasible_step(tri, torch.zeros_like(tri.node_coords_free), eta=eta)
    with pytest.raises(ValueError):
        radapt.RAdaptiveSolver(tri, lf, history=-1)
    with pytest.raises(ValueError):
        radapt.RAdaptiveSolver(tri, lf, quality_weight=-1.0)
    if not torch.cuda.is_available():
        for fn in (radapt.mesh_quality, lambda m: radapt.RAdaptiveSolver(m, lf)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(tri)


# ---------------------------------------------------------------- the numpy oracles of the measure and the step bound
def _measure_np(X, Xref, conn):
    P, R = X[conn], Xref[conn]
    det = lambda T: (T[:, 0, 0] - T[:, 2, 0]) * (T[:, 1, 1] - T[:, 2, 1]) - (T[:, 1, 0] - T[:, 2, 0]) * (T[:, 0, 1] - T[:, 2, 1])
    d, dr = det(P), det(R)
    S = sum(((P[:, (i + 1) % 3] - P[:, i]) ** 2).sum(axis=1) for i in range(3))
    q = 2.0 * math.sqrt(3.0) * np.sign(dr) * d / S
    return q, d / dr


def step_bound_np(X, D, eta):
    """Per element: the smallest alpha > 0 with detJ(X + alpha D) = eta detJ(X) (inf if none; 0 if detJ(X) = 0).  X, D: [Ne, 3, 2]
    corner rows.  The same closed form as csrc/hfem_mesh_elem_dev.h, written independently over arrays."""
    a = X[:, 0] - X[:, 2]
    b = X[:, 1] - X[:, 2]
    da = D[:, 0] - D[:, 2]
    db = D[:, 1] - D[:, 2]
    A0 = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
    A1 = (a[:, 0] * db[:, 1] + da[:, 0] * b[:, 1]) - (b[:, 0] * da[:, 1] + db[:, 0] * a[:, 1])
    A2 = da[:, 0] * db[:, 1] - db[:, 0] * da[:, 1]
    out = np.full(A0.shape, np.inf)
    for i in range(A0.size):
        if A0[i] == 0.0:
            out[i] = 0.0
            continue
        sg = 1.0 if A0[i] > 0 else -1.0
        c, bb, aa = (1.0 - eta) * A0[i] * sg, A1[i] * sg, A2[i] * sg
        disc = bb * bb - 4.0 * aa * c
        if disc < 0.0:
            continue
        sq = math.sqrt(disc)
        if bb < 0.0:
            out[i] = c / (0.5 * (sq - bb))
        elif aa < 0.0:
            out[i] = (-0.5 * (bb + sq)) / aa
    return out, A0, A1, A2


def _scan(A0, A1, A2, eta, amax=50.0, n=400001):
    """First alpha on a fine grid where (detJ(alpha) - eta detJ(0)) changes sign or touches 0, refined by bisection."""
    al = np.linspace(0.0, amax, n)
    f = lambda t: (A0 + A1 * t + A2 * t * t - eta * A0) * np.sign(A0)
    v = f(al)
    hit = np.nonzero(v[1:] <= 0.0)[0]
    if hit.size == 0:
        k = int(np.argmin(v))
        return (np.inf, al[k]) if v[k] > 1e-9 * abs(A0) else (al[k], al[k])
    lo, hi = al[hit[0]], al[hit[0] + 1]
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0.0 else (lo, mid)
    return hi, None


def test_numpy_step_bound_agrees_with_a_brute_force_scan_on_random_triangles():
    rng = np.random.default_rng(0)
    n = 300
    X = rng.normal(size=(n, 3, 2))
    D = rng.normal(size=(n, 3, 2)) * rng.uniform(0.05, 2.0, size=(n, 1, 1))
    eta = 0.25
    got, A0, A1, A2 = step_bound_np(X, D, eta)
    kinds = set()
    for i in range(n):
        want, _ = _scan(A0[i], A1[i], A2[i], eta)
        if np.isinf(want):
            kinds.add("none")
            assert np.isinf(got[i]) or got[i] > 50.0, (i, got[i])
        else:
            kinds.add("root")
            assert abs(got[i] - want) <= 1e-9 * max(1.0, want), (i, got[i], want)
    assert kinds == {"none", "root"}


def test_numpy_step_bound_linear_double_root_zero_direction_and_single_node_cases():
    eta = 0.25
    X = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])          # detJ = (0-0)(0-1) - (1-0)(0-1) = 1
    # d = 0 everywhere: no crossing
    got, *_ = step_bound_np(X, np.zeros_like(X), eta)
    assert np.isinf(got[0])
    # one node pushed straight at its opposite edge: detJ linear in alpha (A2 = 0), crossing at (1 - eta) of the height
    D = np.zeros_like(X)
    D[0, 2] = [0.5, -1.0]                                           # node 2 = (0, 1) moves down toward edge 0-1 (y = 0)
    got, A0, A1, A2 = step_bound_np(X, D, eta)
    assert A2[0] == 0.0 and abs(got[0] - (1.0 - eta)) <= 1e-15
    want, _ = _scan(A0[0], A1[0], A2[0], eta)
    assert abs(got[0] - want) <= 1e-9
    # moving away from the edge: never crosses
    got, *_ = step_bound_np(X, -D, eta)
    assert np.isinf(got[0])
    # a rigid translation keeps detJ: no crossing; a pure rotation rate d = (-y, x) gives detJ(alpha) = (1 + alpha^2) detJ
    got, *_ = step_bound_np(X, np.broadcast_to([0.3, -0.7], X.shape).copy(), eta)
    assert np.isinf(got[0])
    got, *_ = step_bound_np(X, np.stack([-X[..., 1], X[..., 0]], axis=-1), eta)
    assert np.isinf(got[0])
    # uniform shrinking toward the origin, d = -X: detJ(alpha) = (1 - alpha)^2 detJ, first crossing at 1 - sqrt(eta)
    got, *_ = step_bound_np(X, -X, eta)
    assert abs(got[0] - (1.0 - math.sqrt(eta))) <= 1e-15
    # an exact double root: D0 = (15/8, 0), D1 = (0, 5/8) give A1 = -15/8, A2 = 75/64, so detJ(alpha) - eta detJ(0) =
    # 3/4 (1 - alpha / 0.8)^2 touches zero at alpha = 0.8 without crossing (all values binary-exact: disc = 0 exactly)
    D = np.array([[[1.875, 0.0], [0.0, 0.625], [0.0, 0.0]]])
    got, A0, A1, A2 = step_bound_np(X, D, eta)
    assert (A0[0], A1[0], A2[0]) == (1.0, -1.875, 1.171875)
    assert A1[0] ** 2 - 4.0 * A2[0] * (1.0 - eta) * A0[0] == 0.0
    assert abs(got[0] - 0.8) <= 1e-15
    want, _ = _scan(A0[0], A1[0], A2[0], eta, amax=2.0)
    assert abs(want - 0.8) <= 1e-4
    # a degenerate element: no share of nothing can be kept
    got, *_ = step_bound_np(np.array([[[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]]]), np.ones((1, 3, 2)), eta)
    assert got[0] == 0.0
