"""The numpy / scipy reference of the topology-optimisation tests (tests/topopt_reference.py) checked against itself, without a
GPU: the analytic compliance sensitivity against central differences of the sparse-solve compliance, the filter's row sums
and adjointness, and the reference design loop under the conditions the GPU loop test (tests/test_gpu_topopt.py) relies on.

Plates: 12 x 6 of each element kind for the derivative and filter checks; for the loop the plates of tests/test_gpu_modal.py
(23 x 17 TRI3, 23 x 19 QUAD4, jitter 0.25) under the example's load -- the loss's default traction (100e3, 0) on the Neumann
edges -- with volume_fraction 0.4, penal 3, filter radius 1.5 mean element sizes, move 0.2, 60 halvings, 25 iterations.

Central differences with h = 1e-5 on c(rho): truncation h^2 |c'''| / 6 with |c'''| ~ (penal / rho)^2 |dc| <= 1e2 |dc| gives
1e-8 |dc|; rounding eps c / h ~ 1e-11 c with c <= 1e3 max|dc| on these plates gives 1e-8 max|dc|.  Bound: 1e-6 max|dc|."""
import functools

import numpy as np
import pytest
import torch

import topopt_reference as TR

F64 = torch.float64
CONVS = ["reference", "physical"]


@functools.lru_cache(maxsize=None)
def plate(kind, nx, ny, conv, jitter=0.25):
    """Everything the reference needs of one plate, from the mesh generator and a CPU loss: built once, never modified."""
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    gen = structured_quad_mesh if kind == "quad4" else structured_tri_mesh
    nc, conn, geom, bc, mn, edges = gen(nx, ny, jitter=jitter, dtype=F64)
    lf = EnergyLoss2D(device=torch.device("cpu"), dtype=F64, grad_convention=conv)
    X, cn = nc.numpy().astype(np.float64), conn.numpy().astype(np.int64)
    bc = bc.numpy().astype(bool)
    node_row = -np.ones(X.shape[0], dtype=np.int64)
    node_row[~bc] = np.arange(int((~bc).sum()))
    Ke = TR.element_matrices(X, cn, lf._mat, lf._W, conv)
    dofs = TR.element_dofs(cn, node_row)
    cen, vol = TR.geometry(X, cn)
    f = TR.edge_load(X, edges.numpy(), node_row, (100e3, 0.0), lf._ci, lf._cj)   # the loss's own edge rule
    return dict(Ke=Ke, dofs=dofs, n_free=2 * int((~bc).sum()), cen=cen, vol=vol, f=f)


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_analytic_sensitivity_against_central_differences(kind, conv):
    P = plate(kind, 12, 6, conv)
    rng = np.random.default_rng(3)
    ne = len(P["vol"])
    rho = rng.uniform(0.3, 0.9, ne)
    F = TR.filter_matrix(P["cen"], P["vol"], 1.5 * np.sqrt(P["vol"].mean()))
    penal, e_min, h = 3.0, 1e-3, 1e-5
    c, dc, _, _ = TR.compliance_and_sensitivity(P["Ke"], P["dofs"], P["n_free"], P["f"], rho, F, penal, e_min)
    assert c > 0 and (dc < 0).all()
    worst = 0.0
    for e in rng.choice(ne, 8, replace=False):
        rp, rm = rho.copy(), rho.copy()
        rp[e] += h
        rm[e] -= h
        cp = TR.compliance_and_sensitivity(P["Ke"], P["dofs"], P["n_free"], P["f"], rp, F, penal, e_min)[0]
        cm = TR.compliance_and_sensitivity(P["Ke"], P["dofs"], P["n_free"], P["f"], rm, F, penal, e_min)[0]
        worst = max(worst, abs((cp - cm) / (2 * h) - dc[e]) / np.abs(dc).max())
    print(f"{kind} {conv}: c {c:.4e} max|dc| {np.abs(dc).max():.3e} worst |fd - dc| / max|dc| {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_filter_rows_sum_to_one_and_the_transpose_is_the_adjoint(kind):
    P = plate(kind, 12, 6, "physical")
    cen, vol = P["cen"], P["vol"]
    r = 1.5 * np.sqrt(vol.mean())
    F = TR.filter_matrix(cen, vol, r)
    assert np.abs(F.sum(axis=1) - 1.0).max() <= 1e-14 and (F >= 0).all()
    # the transpose by its own formula, out_j = v_j sum_e H_je in_e / s_e (H symmetric), against <y, F x> = <F^T y, x>
    d = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2))
    H = np.maximum(0.0, r - d)
    assert np.array_equal(H, H.T)
    s = H @ vol
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(len(vol)), rng.standard_normal(len(vol))
    ty = vol * (H @ (y / s))
    assert abs(y @ (F @ x) - ty @ x) <= 1e-13 * np.abs(y).sum() * np.abs(x).max()
    assert np.abs(ty - F.T @ y).max() <= 1e-14 * np.abs(y).max() * len(vol)
    assert np.array_equal(TR.filter_matrix(cen, vol, 0.0), np.eye(len(vol)))


LOOP = dict(volume_fraction=0.4, penal=3.0, e_min=1e-9, move=0.2, n_bisect=60, n_iter=25)


@functools.lru_cache(maxsize=None)
def reference_loop(kind, conv="physical"):
    """The reference design loop on the plate of tests/test_gpu_modal.py: computed once, shared, never modified."""
    P = plate(kind, 23, 19 if kind == "quad4" else 17, conv)
    F = TR.filter_matrix(P["cen"], P["vol"], 1.5 * np.sqrt(P["vol"].mean()))
    cs, vs, fl, rho = TR.oc_loop(P["Ke"], P["dofs"], P["n_free"], P["f"], P["vol"], F, **LOOP)
    return P, F, cs, vs, fl, rho


@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_reference_loop_meets_the_volume_target_and_decreases_the_compliance(kind):
    P, F, cs, vs, fl, rho = reference_loop(kind)
    ne = len(P["vol"])
    target = LOOP["volume_fraction"] * P["vol"].sum()
    err = np.abs(vs - target).max() / target
    print(f"{kind}: c_1 {cs[0]:.4e} c_25 {cs[-1]:.4e} ratio {cs[-1] / cs[0]:.3f} monotone {bool((np.diff(cs) < 0).all())} "
          f"volume error {err:.1e}")
    assert all(fl)
    assert (vs <= target * (1 + 4 * ne * 2.0 ** -53)).all()
    assert err <= 1e-9                                       # 60 halvings of [0, R]: the bracket is R 2^-60 wide
    assert (rho >= 0).all() and (rho <= 1).all()
    assert (np.diff(cs) < 0).all(), cs
    assert cs[-1] <= 0.5 * cs[0]
