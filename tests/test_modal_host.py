"""The modal solver's host surface, without a GPU: the new C entry points are exported, bound and match the header, argument
errors come back as negative codes with a message before any device is touched, ``ModalSolver`` refuses what it does not
support, and the host Ritz step (numpy) solves a small pencil."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

MODAL_SYMBOLS = ["hfem_mass_apply", "hfem_block_gram", "hfem_block_combine", "hfem_block_residual", "hfem_block_jacobi_apply"]


def _lib():
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.csrc import build
    build.build()
    return _lib


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "hidenn_fem.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(hfem_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_modal_symbols_are_exported_bound_and_match_the_header():
    L = _lib()
    h = C.CDLL(L.LIB_PATH)
    counts = _header_arg_counts()
    for n in MODAL_SYMBOLS:
        assert hasattr(h, n), n
        assert n in L.PROTOTYPES, n
        assert n in counts, f"{n} is not declared in include/hidenn_fem.h"
        assert getattr(L.lib(), n).argtypes == L.PROTOTYPES[n][1]
        assert len(L.PROTOTYPES[n][1]) == counts[n], n
    assert L.lib().hfem_version() == 114
    from hidenn_fem_amd import modal
    text = open(os.path.join(ROOT, "include", "hidenn_fem.h")).read()
    assert f"#define HFEM_BLOCK_GRAM_PARTIALS {modal.GRAM_PARTIALS}\n" in text
    assert f"#define HFEM_BLOCK_RESIDUAL_PARTIALS {modal.RESIDUAL_PARTIALS}\n" in text
    from hidenn_fem_amd.csrc import build
    assert "modal.hip" in build.SOURCES


def test_modal_argument_errors_are_negative_codes_with_messages():
    lib = _lib().lib()
    err = lib.hfem_last_error
    buf = (C.c_double * 64)()
    idx = (C.c_int32 * 16)()
    p, q = C.addressof(buf), C.addressof(idx)
    mass = lambda device=0, npe=3, X=p, m=1, V=p, MV=p + 128, rho=1.0: lib.hfem_mass_apply(
        device, npe, X, q, 1, 3, q, q, q, q, 3, rho, 0, V, m, MV, None)
    assert mass(X=None) < 0 and b"hfem_mass_apply: null pointer" in err()
    assert mass(npe=5) < 0 and b"npe" in err()
    assert mass(m=0) < 0 and b"1..8" in err()
    assert mass(m=9) < 0 and b"1..8" in err()
    assert mass(device=-1) < 0 and b"negative device" in err()
    assert mass(MV=p) < 0 and b"alias" in err()
    assert mass(rho=0.0) < 0 and b"rho" in err()
    assert lib.hfem_block_gram(0, None, 1, p, 1, 2, p, p, None) < 0 and b"hfem_block_gram: null pointer" in err()
    assert lib.hfem_block_gram(0, p, 25, p, 1, 2, p, p, None) < 0 and b"1..24" in err()
    assert lib.hfem_block_gram(0, p, 1, p, 0, 2, p, p, None) < 0 and b"1..24" in err()
    assert lib.hfem_block_gram(0, p, 1, p, 1, 3, p, p, None) < 0 and b"even" in err()
    assert lib.hfem_block_gram(-2, p, 1, p, 1, 2, p, p, None) < 0 and b"negative device" in err()
    assert lib.hfem_block_combine(0, p, 1, None, 1, 2, p + 64, None) < 0 and b"hfem_block_combine: null pointer" in err()
    assert lib.hfem_block_combine(0, p, 25, p, 1, 2, p + 64, None) < 0 and b"1..24" in err()
    assert lib.hfem_block_combine(0, p, 2, p, 2, 4, p + 32, None) < 0 and b"overlap" in err()        # S is 8 doubles long
    assert lib.hfem_block_combine(-1, p, 1, p, 1, 2, p + 64, None) < 0 and b"negative device" in err()
    assert lib.hfem_block_residual(0, p, p, None, 1, 2, p, p, p, None) < 0 and b"hfem_block_residual: null pointer" in err()
    assert lib.hfem_block_residual(0, p, p, p, 9, 2, p, p, p, None) < 0 and b"1..8" in err()
    assert lib.hfem_block_residual(-1, p, p, p, 1, 2, p, p, p, None) < 0 and b"negative device" in err()
    assert lib.hfem_block_jacobi_apply(0, None, p, 1, 2, p, None) < 0 and b"hfem_block_jacobi_apply: null pointer" in err()
    assert lib.hfem_block_jacobi_apply(0, p, p, 0, 2, p, None) < 0 and b"1..8" in err()
    assert lib.hfem_block_jacobi_apply(-1, p, p, 1, 2, p, None) < 0 and b"negative device" in err()


def _model(quad=False, dirichlet=True, n=(7, 5)):
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    gen, cls = (structured_quad_mesh, QuadShapeNN2D) if quad else (structured_tri_mesh, PiecewiseLinearShapeNN2D)
    nc, conn, geom, bc, mn, edges = gen(*n, dtype=torch.float64)
    return cls(nc, conn, boundary_mask=geom, dirichlet_mask=bc if dirichlet else None, u_fixed=0.0, neumann_edges=edges)


def test_modal_solver_refuses_what_it_does_not_support():
    from hidenn_fem_amd.loss import EnergyLoss2D, NeoHookeanLoss2D
    from hidenn_fem_amd.modal import ModalSolver, vibration_modes
    cpu = torch.device("cpu")
    lf = EnergyLoss2D(device=cpu, dtype=torch.float64)
    for quad in (False, True):
        with pytest.raises(ValueError, match="Dirichlet rows"):
            ModalSolver(_model(quad, dirichlet=False), lf)
    with pytest.raises(NotImplementedError, match="NeoHookeanLoss2D"):
        ModalSolver(_model(), NeoHookeanLoss2D(device=cpu, dtype=torch.float64))
    for kw in (dict(n_modes=0), dict(n_modes=9), dict(n_modes=4, block=3), dict(n_modes=2, block=9)):
        with pytest.raises(ValueError, match="n_modes <= block <= 8"):
            ModalSolver(_model(), lf, **kw)
    with pytest.raises(ValueError, match="mass"):
        ModalSolver(_model(), lf, mass="diagonal")
    with pytest.raises(ValueError, match="precond"):
        ModalSolver(_model(), lf, precond="none")
    with pytest.raises(ValueError, match="density"):
        ModalSolver(_model(), lf, density=0.0)
    small = _model(n=(3, 3))                                 # 9 nodes, 3 of them fixed: 12 free dofs < 3 x 8
    assert 2 * small.u_free.shape[0] < 24
    with pytest.raises(ValueError, match="3 x block"):
        ModalSolver(small, lf, n_modes=6)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ModalSolver(_model(), lf)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            vibration_modes(_model(quad=True), lf, n_modes=2)


def test_the_product_does_not_import_scipy():
    import subprocess
    import sys
    code = "import sys; import hidenn_fem_amd.modal; assert 'scipy' not in sys.modules, 'scipy imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_host_ritz_step_and_its_safeguards():
    from hidenn_fem_amd.modal import rayleigh_ritz
    rng = np.random.default_rng(3)
    n, ms = 40, 9
    A = rng.standard_normal((n, n))
    K, M = A @ A.T + n * np.eye(n), np.diag(rng.uniform(1.0, 2.0, n))
    S = rng.standard_normal((n, ms)) * 10.0 ** rng.integers(-8, 3, ms)          # columns of very different size
    lam, Cm, dropped = rayleigh_ritz(S.T @ K @ S, S.T @ M @ S, 4)
    X = S @ Cm
    assert dropped == 0
    assert np.abs(X.T @ M @ X - np.eye(4)).max() <= 1e-10
    assert np.abs(X.T @ K @ X - np.diag(lam)).max() <= 1e-9 * lam.max() and (np.diff(lam) >= 0).all()
    Q = np.linalg.qr(S / np.linalg.norm(S, axis=0))[0]                         # the same span, orthonormal columns
    Li = np.linalg.inv(np.linalg.cholesky(Q.T @ M @ Q))
    ref = np.linalg.eigvalsh(Li @ (Q.T @ K @ Q) @ Li.T)[:4]
    assert np.abs(lam - ref).max() <= 1e-8 * ref.max()
    # a dependent column (the last one): with every column required the step is refused; with X = the first three required
    # it is left out, its coefficients are zero and the step is the one on the other five
    S2 = np.concatenate([S[:, :5], S[:, :1] + 1e-9 * S[:, 1:2]], axis=1)
    gk, gm = S2.T @ K @ S2, S2.T @ M @ S2
    assert rayleigh_ritz(gk, gm, 3) is None
    lam2, C2, dropped = rayleigh_ritz(gk, gm, 3, n_required=3, order=[0, 1, 2, 5, 3, 4])
    lam5, C5, _ = rayleigh_ritz(gk[:5, :5], gm[:5, :5], 3)
    assert dropped == 1 and (C2[5] == 0.0).all() and (C2[3] != 0.0).any() and (C2[4] != 0.0).any()
    assert np.abs(lam2 - lam5).max() <= 1e-9 * lam5.max()                       # the same span
    # the dependent column among the required ones: refused
    assert rayleigh_ritz(gk, gm, 3, n_required=4, order=[1, 2, 0, 5, 3, 4]) is None
    assert rayleigh_ritz(np.full((2, 2), np.nan), np.eye(2), 1) is None
    assert rayleigh_ritz(np.eye(2), np.diag([1.0, -1.0]), 1) is None
    lam1, C1, dropped = rayleigh_ritz(np.eye(2), np.diag([1.0, -1.0]), 1, n_required=1)
    assert dropped == 1 and lam1[0] == 1.0 and C1[1, 0] == 0.0


def test_ritz_step_on_nearly_dependent_p_and_w():
    """The solver's own call -- ``[X P W]`` walked X, W, P with X required -- on bases whose W and P columns depend on X and on
    each other to 1e-3 ... 1e-12: the step is never refused (X is M-orthonormal, so its pivots are 1), the new X is
    M-orthonormal, and its Ritz values lie between the pencil's eigenvalues and those of the old X (Cauchy interlacing: the new
    span contains the old X).  M-orthonormality to 24 eps / PIVOT_TOL^2: the Gram matrix of the kept columns has pivots of at
    least PIVOT_TOL, so its condition is at most about ms / PIVOT_TOL^2, and C^T G C = I holds to eps times that."""
    from hidenn_fem_amd.modal import PIVOT_TOL, rayleigh_ritz
    rng = np.random.default_rng(17)
    n, b = 60, 4
    A = rng.standard_normal((n, n))
    K, M = A @ A.T + n * np.eye(n), np.diag(rng.uniform(1.0, 2.0, n))
    Lm = np.sqrt(np.diag(M))
    true = np.linalg.eigvalsh(K / Lm[:, None] / Lm[None, :])
    tol = 24 * np.finfo(float).eps / PIVOT_TOL ** 2
    left_out = 0
    for trial in range(200):
        X = rng.standard_normal((n, b))
        l0, C0, _ = rayleigh_ritz(X.T @ K @ X, X.T @ M @ X, b)
        X = X @ C0
        near = lambda: X @ rng.standard_normal((b, b)) + 10.0 ** rng.integers(-12, -2, b) * rng.standard_normal((n, b))
        W = near() * 10.0 ** rng.integers(-9, 1, b)
        P = np.where(rng.random(b) < 0.5, near(), W @ rng.standard_normal((b, b)) + 1e-9 * rng.standard_normal((n, b)))
        S = np.concatenate([X, P, W], axis=1)
        order = list(range(b)) + list(range(2 * b, 3 * b)) + list(range(b, 2 * b))
        rr = rayleigh_ritz(S.T @ K @ S, S.T @ M @ S, b, n_required=b, order=order)
        assert rr is not None, trial
        lam, Cm, dropped = rr
        left_out += dropped
        Xn = S @ Cm
        assert np.abs(Xn.T @ M @ Xn - np.eye(b)).max() <= tol, trial
        assert (lam <= l0 * (1 + 1e-9)).all() and (lam >= true[:b] * (1 - 1e-9)).all(), trial
    assert left_out > 0                                      # the safeguard was at work
