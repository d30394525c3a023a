"""tests/hyper_dynamics_reference.py pinned on its own, on the CPU: the Jacobian and the incremental potential against central
differences of the residual, the small-load limit against the linear Newmark step of tests/dynamics_reference.py, and the
explicit step against the general one.  The 17 x 9 plates of the static Newton tests (E = 2e6, left edge clamped, the default
traction on the right edge), rho = 2."""
import numpy as np
import pytest
import torch

import dynamics_reference as DR
import hyper_dynamics_reference as HD
import newton_reference as N
import quad4_newton_reference as QN

RHO = 2.0
LOAD = 0.01                   # of the default traction (a step load's first acceleration sits in the loaded edge alone)
_cache = {}


def system(kind, lumped=False):
    """The plate with its edge loads as ``b`` and without them as the internal problem; computed once, never modified."""
    key = (kind, lumped)
    if key not in _cache:
        mod = QN if kind == "quad4" else N
        b = HD.external_load(mod.plate_problem())
        _cache[key] = HD.System(mod.plate_problem(loads=False), b, rho=RHO, lumped=lumped)
    return _cache[key]


def period(sys):
    import scipy.linalg
    w = scipy.linalg.eigh(sys.K_T(np.zeros(2 * sys.n)), sys.M, eigvals_only=True, subset_by_index=[0, 0])
    return 2 * np.pi / np.sqrt(w[0])


def state(sys, dt, seed=3):
    """A deformed, moving point to differentiate at: the predictor (u~, v~) of the fourth step of the loaded plate from rest
    and that step's solution a+ (so u~ + c_K a+ is a state the plate really takes).  -> (u~, v~, a+, rng)"""
    u, v = np.zeros(2 * sys.n), np.zeros(2 * sys.n)
    a = HD.initial_acceleration(sys, u, v, load0=LOAD)
    for k in range(4):
        ut, vt = HD.predictor(u, v, a, dt)
        u, v, a, _, min_j = HD.step(sys, u, v, a, dt, LOAD)
        assert 0.5 < min_j < 1.5
    return ut, vt, a, np.random.default_rng(seed)


@pytest.mark.parametrize("alpha_r", [0.0, 0.7])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_jacobian_and_potential_against_central_differences(kind, alpha_r):
    """Directional derivatives along three random directions w: J w against (R(a + h w) - R(a - h w))
    / 2h and c_K R . w against (Phi(a + h w) - Phi(a - h w)) / 2h.  Central differences are second order: from h to h / 2 the
    error falls by 4 (asserted: between 3 and 5; h is chosen where truncation, not rounding, is what is left)."""
    sys = system(kind)
    dt = period(sys) / 20
    ut, vt, a, rng = state(sys, dt)
    kw = dict(alpha_r=alpha_r)
    c_k, _ = HD.coefficients(dt, alpha_r=alpha_r)
    scale = 0.01 / c_k                                     # h w moves the nodes by up to h / 200 of the plate's side
    a = a + 0.5 * scale * (rng.random(a.shape) - 0.5)      # off the step's solution, where R = 0
    J = HD.jacobian(sys, a, ut, dt, **kw)
    R = HD.residual(sys, a, ut, vt, dt, LOAD, **kw)
    for _ in range(3):
        w = scale * (rng.random(a.shape) - 0.5)
        assert np.abs(J - J.T).max() <= 1e-12 * np.abs(J).max()
        errs_j, errs_p = [], []
        for h in (HJ, HJ / 2):
            fd = (HD.residual(sys, a + h * w, ut, vt, dt, LOAD, **kw) - HD.residual(sys, a - h * w, ut, vt, dt, LOAD, **kw)) / (2 * h)
            errs_j.append(np.linalg.norm(fd - J @ w) / np.linalg.norm(J @ w))
        for h in (HP, HP / 2):
            fd = (HD.potential(sys, a + h * w, ut, vt, dt, LOAD, **kw) - HD.potential(sys, a - h * w, ut, vt, dt, LOAD, **kw)) / (2 * h)
            errs_p.append(abs(fd - c_k * (R @ w)) / abs(c_k * (R @ w)))
        print(kind, alpha_r, "J", errs_j, errs_j[0] / errs_j[1], "Phi", errs_p, errs_p[0] / errs_p[1])
        assert errs_j[0] <= 0.1 and 3.0 <= errs_j[0] / errs_j[1] <= 5.0
        assert errs_p[0] <= 0.1 and 3.0 <= errs_p[0] / errs_p[1] <= 5.0


HJ, HP = 0.25, 0.25           # nodes move by up to 1.25e-3, 2 % of an element's side (the printed errors: ~1e-3, far above rounding)


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_small_loads_approach_the_linear_step(kind):
    """f_int(u) = K_T(0) u + O(u^2): with the load scaled by eps the finite-strain step and the linear step on K_T(0) differ by
    O(eps^2), relative to the O(eps) answer by O(eps).  eps = 1e-2 and 1e-3 (strains of 1e-3 and 1e-4 on this plate: far above
    rounding, far below the radius where the next order shows): the relative difference falls by 10 (asserted: 5 to 20)."""
    sys = system(kind)
    dt = period(sys) / 20
    K0 = sys.K_T(np.zeros(2 * sys.n))
    rel = []
    for eps in (EPS_LOAD, EPS_LOAD / 10):
        u, v = np.zeros(2 * sys.n), np.zeros(2 * sys.n)
        a = HD.initial_acceleration(sys, u, v, load0=eps)
        ul, vl, al = u.copy(), v.copy(), a.copy()
        for _ in range(3):
            u, v, a = HD.step(sys, u, v, a, dt, eps)[:3]
            ul, vl, al = DR.step(K0, sys.M, sys.b, ul, vl, al, dt, eps)
        rel.append(np.linalg.norm(a - al) / np.linalg.norm(al))
    print(kind, "relative difference", rel, rel[0] / rel[1])
    assert rel[0] <= 0.1 and 5.0 <= rel[0] / rel[1] <= 20.0


EPS_LOAD = 1e-2


@pytest.mark.parametrize("alpha_r", [0.0, 0.7])
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_lumped_beta_zero_is_the_explicit_step(kind, alpha_r):
    sys = system(kind, lumped=True)
    w_max = np.sqrt(np.linalg.eigvalsh(np.linalg.solve(sys.M, sys.K_T(np.zeros(2 * sys.n)))).max())
    dt = 1.0 / w_max                                       # half the critical step 2 / w_max
    u, v = np.zeros(2 * sys.n), np.zeros(2 * sys.n)
    a = HD.initial_acceleration(sys, u, v, alpha_r)
    for k in range(5):
        ue, ve, ae, _ = HD.explicit_step(sys, u, v, a, dt, 1.0, alpha_r=alpha_r)
        u, v, a, rn, _ = HD.step(sys, u, v, a, dt, 1.0, beta=0.0, alpha_r=alpha_r)
        for x, y in ((u, ue), (v, ve), (a, ae)):
            assert np.linalg.norm(x - y) <= 1e-13 * np.linalg.norm(y)
