"""CPU checks of tests/pointwise_cases.py: the builders have the properties tests/test_gpu_pointwise_edges.py relies on, and
the references it compares a kernel with agree with each other."""
import numpy as np
import torch

import pointwise_cases as K
from conftest import tri_mesh_dict
from oracle import closed_form as CF
from oracle import ref_chain as R

F64 = torch.float64


def _det(c, ids=None):
    ids = torch.arange(c["conn"].shape[0]) if ids is None else ids
    return R.tri3_forward(c["X"], c["U"], c["conn"], torch.zeros((ids.shape[0], 2), dtype=F64), ids)[1]


def _grad_close(got, want, what):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert (got - want).abs().max() <= K.GRAD_RTOL * want.abs().max(), what


def test_size_lists_follow_the_grid_caps():
    assert K.POINT_M == (1, 255, 256, 257, 2048 * 256 + 1)
    assert K.ENERGY_N == (1, 257, 2048 * 256 + 1) and K.QUAD4_N == (1, 257, 4096 * 256 + 1)
    assert K.POST_N == (1, 256, 257, 8192 * 256 + 1)
    for w in K.ROW_WIDTHS:
        assert K.row_counts(w)[-1] * w > K.EVAL_CAP >= (K.row_counts(w)[-1] - 1) * w
        assert (K.slope_nodes(w)[-1] - 1) * w > K.POST_CAP and K.slope_nodes(w)[:4] == (0, 1, 2, 257)
    assert K.NCX <= 12 and K.NCY <= 9 and K.ONE_ELEMENT_M >= 4096


def test_both_orientations_are_present_and_sampled():
    c = K.tri3_case("arange")
    det = _det(c)
    ne = det.shape[0]
    assert int((det < 0).sum()) == len(range(1, ne, K.FLIP_EVERY)) and int((det > 0).sum()) == ne - int((det < 0).sum())
    assert (det.abs() > 0.02).all()                                   # no element is near degenerate on this mesh
    for ids, m in [("multiset", m) for m in K.POINT_M[1:]] + [("special", None), ("arange", None)]:
        d = _det(c, K.tri3_case(ids, m)["elem_id"])
        assert (d < 0).any() and (d > 0).any(), (ids, m)
    assert det[K.ONE_ELEMENT] < 0                                     # the all-in-one-element case sits in a clockwise one
    q = K.quad_mesh()
    import oracle.quad4 as Q4
    dq = Q4.quad4_forward(q["X"], c["U"], q["conn"], torch.zeros((q["conn"].shape[0], 2), dtype=F64), torch.arange(q["conn"].shape[0]))[1]
    assert (dq < 0).any() and (dq > 0).any()


def test_repeats_have_the_stated_multiplicity():
    c = K.tri3_case("one", K.ONE_ELEMENT_M)
    assert c["elem_id"].shape[0] == K.ONE_ELEMENT_M >= 4096 and (c["elem_id"] == K.ONE_ELEMENT).all()
    ne, ned = K.tri_mesh()["conn"].shape[0], K.tri_mesh()["edges"].shape[0]
    for m in K.POINT_M[1:]:
        cnt = torch.bincount(K.tri3_case("multiset", m)["elem_id"], minlength=ne)
        assert cnt.max() >= 2 and cnt.sum() == m and (m < 10 * ne or cnt.min() >= 1)
        cnt = torch.bincount(K.edge2_case("multiset", m)["edge_id"], minlength=ned)
        assert cnt.max() >= 2 and cnt.sum() == m and cnt.min() >= 1
    assert (K.edge2_case("one", K.ONE_ELEMENT_M)["edge_id"] == K.ONE_EDGE).all()
    mc = K.model_case()
    assert torch.bincount(mc["elem_id"], minlength=ne).min() >= 5 and torch.bincount(mc["edge_id"], minlength=ned).min() >= 50
    assert torch.arange(ne).equal(K.tri3_case("arange")["elem_id"])
    for with_boundary in (True, False):                               # every gradient of the model cases reaches a free row
        w = K.model_expected(mc, with_boundary=with_boundary)
        assert all(g.abs().max() > 0 for g in w["tri"][3:] + w["edge"][2:])
    assert mc["boundary_mask"].any() and not mc["boundary_mask"].all() and mc["dirichlet_mask"].any()
    for n in (K.ENERGY_N[-1],):
        conn = K.repeated(K.tri_mesh()["conn"], n)
        assert conn.shape == (n, 3) and conn[ne:2 * ne].equal(K.tri_mesh()["conn"]) and conn[-1].equal(K.tri_mesh()["conn"][(n - 1) % ne])


def test_vertex_edge_and_outside_points_are_present():
    c = K.tri3_case("special")
    w = K.barycentric(c["x_eval"][:len(K.SPECIAL)])
    vertex = ((w == 1).sum(dim=1) == 1) & ((w == 0).sum(dim=1) == 2)
    edge = ((w == 0).sum(dim=1) == 1) & ((w == 0.5).sum(dim=1) == 2)
    outside = (w < 0).any(dim=1)
    assert int(vertex.sum()) == 3 and int(edge.sum()) == 3 and int(outside.sum()) == 4
    assert {int(i) for i in w[vertex].argmax(dim=1)} == {0, 1, 2} and {int(i) for i in w[edge].argmin(dim=1)} == {0, 1, 2}
    assert (w[outside] < 0).any(dim=0).all() and (w[outside] > 1).any(dim=0)[[0, 2]].all()    # each weight negative somewhere; r.x, zeta > 1
    assert int((~(vertex | edge | outside)).sum()) == 1               # the centroid
    assert c["elem_id"].shape[0] == len(K.SPECIAL) * K.tri_mesh()["conn"].shape[0]
    for m in K.POINT_M[1:]:
        w = K.barycentric(K.tri3_case("multiset", m)["x_eval"])
        assert (w < 0).any() and (w > 1).any() and ((w > 0).all(dim=1)).any()
    xi = K.edge2_case("special")["xi"][:len(K.XI_SPECIAL)]
    assert (xi == 0).any() and (xi == 1).any() and (xi < 0).any() and (xi > 1).any() and ((xi > 0) & (xi < 1)).any()
    e = K.tri_mesh()["edges"]
    assert {(int(a), int(b)) for a, b in e} == {(int(b), int(a)) for a, b in e}      # every edge in both directions


def test_nodal_values_do_not_cancel_at_outside_points():
    """What the rtol on u_h rests on (module docstring of pointwise_cases): |sum w U| against max |w U| over the largest case."""
    c = K.tri3_case("multiset", K.POINT_M[-1])
    w, Un = K.barycentric(c["x_eval"]), c["U"][c["conn"][c["elem_id"]]]
    terms = w.unsqueeze(2) * Un
    assert (terms.sum(dim=1).abs() >= 0.2 * terms.abs().amax(dim=1)).all()
    mc = K.model_case()
    U = R.assemble_u(mc["X"].shape[0], ~mc["dirichlet_mask"], mc["u_free"], mc["dirichlet_mask"], torch.tensor(K.U_FIXED, dtype=F64))
    terms = K.barycentric(mc["x_eval"]).unsqueeze(2) * U[mc["conn"][mc["elem_id"]]]
    assert (terms.sum(dim=1).abs() >= 0.1 * terms.abs().amax(dim=1)).all()


def test_degenerate_element_has_the_stated_aspect():
    c = K.degenerate_case()
    X = c["X"]
    det = _det(c)[0].abs().item()
    edges = [(X[i] - X[j]).norm().item() for i, j in ((0, 1), (1, 2), (2, 0))]
    aspect = max(edges) ** 2 / det                                    # longest edge over the height on it
    assert 5e5 <= aspect <= 2e6 and 1e-6 <= det / (edges[1] * edges[2]) <= 1e-5
    a, b = X[0] - X[2], X[1] - X[2]
    assert abs((a[0] * b[1]).item()) > 1e4 * det                      # a d and b c cancel: the turned element, not an aligned one


def test_degenerate_oracle_error_is_the_recorded_one():
    """The fp64 ``ref_chain`` result on the near-degenerate element against the longdouble restatement.  Measured
    (max-abs over the 31 points; relative to the largest entry in brackets):

        convention   detJ                 grad_u               gX                   gU
        reference    1.0046e-18 (1.0e-12) 3.0342e-11 (1.0e-12) 5.5791e-05 (2.0e-12) 4.7266e-07 (1.0e-12)
        physical     1.0046e-18 (1.0e-12) 5.2145e-11 (1.0e-12) 6.6172e-04 (2.0e-12) 7.2264e-06 (1.0e-12)

    against 2.3e-16 for u_h, which keeps its rtol.  The GPU test allows DEGENERATE_FACTOR = 8 times these.  For scale:
    a d = -0.1232, so one rounding of a product (or of an edge difference a, b, c, d, which the oracle and an fp64 kernel
    round alike) is worth up to ulp(0.1232) / 2 / det = 6.9e-12 of det: a kernel that forms det with one fused multiply-add
    on the same edge differences stays inside 8 x 1.0e-12."""
    assert np.finfo(K.LD).eps < 2e-19
    for conv, rec in K.DEGENERATE_REF_ERR.items():
        got = K.degenerate_measured(conv)
        print(conv, got)
        for k, v in rec.items():
            assert 0.5 * v <= got[k] <= 1.001 * v, (conv, k, got[k], v)
    c = K.degenerate_case()
    ref, ld = K.tri3_expected(c), K.tri3_closed_form_ld(c)
    assert K.max_err_ld(ref["u_h"], ld["u_h"]) <= K.U_RTOL * float(np.abs(ld["u_h"]).min())


def test_longdouble_restatement_is_the_oracle_chain():
    """On the well-shaped mesh the longdouble closed form and ``ref_chain`` + autograd agree within the bounds of case A, for
    every cotangent subset and both conventions -- the restatement (its backward above all) states the same function."""
    c = K.tri3_case("multiset", 257)
    for conv in ("reference", "physical"):
        for cots in K.COT_SUBSETS:
            ref, ld = K.tri3_expected(c, conv, cots), K.tri3_closed_form_ld(c, conv, cots)
            f = {k: v.astype(np.float64) for k, v in ld.items()}
            np.testing.assert_allclose(ref["u_h"].numpy(), f["u_h"], rtol=K.U_RTOL)
            np.testing.assert_allclose(ref["detJ"].numpy(), f["detJ"], rtol=K.U_RTOL)
            np.testing.assert_allclose(ref["grad_u"].numpy(), f["grad_u"], rtol=K.GRADU_RTOL, atol=K.GRADU_ATOL)
            for k in ("gX", "gU"):
                if cots and (k, cots) not in (("gX", ("cu",)), ("gU", ("cd",))):
                    _grad_close(ref[k], f[k], (conv, cots, k))
                    assert np.abs(f[k]).max() > 0
                else:                                   # no cotangent; u_h does not depend on X, nor detJ on U
                    assert not f[k].any() and not ref[k].any()
    ref = K.tri3_expected(c, "reference")
    phys = K.tri3_expected(c, "physical")
    assert (ref["grad_u"] - phys["grad_u"]).abs().max() > 1e-3 * ref["grad_u"].abs().max()        # the conventions differ here


def test_closed_form_eval_matches_ref_chain():
    for ids, m in (("special", None), ("multiset", 257), ("one", K.ONE_ELEMENT_M)):
        c = K.tri3_case(ids, m)
        ref = K.tri3_expected_cached(ids, m, "reference")
        u_h, detJ, grad_u = CF.tri3_eval(c["X"].numpy(), c["U"].numpy(), c["conn"].numpy(), c["x_eval"].numpy(), c["elem_id"].numpy())
        np.testing.assert_allclose(u_h, ref["u_h"].numpy(), rtol=K.U_RTOL)
        np.testing.assert_allclose(detJ, ref["detJ"].numpy(), rtol=K.U_RTOL)
        np.testing.assert_allclose(grad_u, ref["grad_u"].numpy(), rtol=K.GRADU_RTOL, atol=K.GRADU_ATOL)


def test_golden_per_point_vectors_match_ref_chain(g_tri):
    mesh, xf, uf = tri_mesh_dict(g_tri, "order4")
    p = "order4/pp_"
    xf, uf = xf.requires_grad_(True), uf.clone().requires_grad_(True)
    X = R.assemble_coords(mesh["n_nodes"], mesh["free_mask"], xf, mesh["boundary_mask"], mesh["coords_fixed"])
    U = R.assemble_u(mesh["n_nodes"], mesh["u_free_mask"], uf, mesh["dirichlet_mask"], mesh["u_fixed"])
    u_h, detJ, grad_u = R.tri3_forward(X, U, mesh["conn"], g_tri.t(p + "x_eval"), g_tri.t(p + "elem_id"))
    np.testing.assert_allclose(u_h.detach().numpy(), g_tri[p + "u_h"], rtol=K.U_RTOL, atol=1e-20)
    np.testing.assert_allclose(detJ.detach().numpy(), g_tri[p + "detJ"], rtol=K.U_RTOL)
    np.testing.assert_allclose(grad_u.detach().numpy(), g_tri[p + "grad_u"], rtol=K.GRADU_RTOL, atol=K.GRADU_ATOL)
    ((u_h * g_tri.t(p + "cu")).sum() + (detJ * g_tri.t(p + "cd")).sum() + (grad_u * g_tri.t(p + "cg")).sum()).backward()
    _grad_close(uf.grad, g_tri[p + "g_u_free"], "golden gU")
    _grad_close(xf.grad, g_tri[p + "g_coords_free"], "golden gX")
    q = "order4/pe_"
    ue, ds = R.edge2_forward(X, U, mesh["edges"], g_tri.t(q + "x_eval"), g_tri.t(q + "edge_id"))
    np.testing.assert_allclose(ue.detach().numpy(), g_tri[q + "u_h"], rtol=K.U_RTOL, atol=1e-20)
    np.testing.assert_allclose(ds.detach().numpy(), g_tri[q + "ds"], rtol=K.U_RTOL)


def test_edge2_ds_gradient_closed_form_matches_autograd():
    for ids, m in (("special", None), ("multiset", 257), ("one", K.ONE_ELEMENT_M)):
        c = K.edge2_case(ids, m)
        both, only_ds, only_u = K.edge2_expected(c), K.edge2_expected(c, ("cd",)), K.edge2_expected(c, ("cu",))
        _grad_close(K.edge2_ds_gradient(c), only_ds["gX"], ids)
        _grad_close(both["gX"], only_ds["gX"], ids)                   # u_h does not depend on X ...
        assert not only_u["gX"].any() and not only_ds["gU"].any()     # ... nor ds on U
        assert only_ds["gX"].abs().max() > 0 and only_u["gU"].abs().max() > 0


def test_energy_statements_are_positive_sums_and_additive():
    """The planless-energy cases: positive element energies (so LOSS_RTOL is asked of a sum without cancellation), additive over
    the ranges the GPU test cuts, and the repeated connectivity is worth the whole multiples plus the remainder."""
    mesh = K.tri_mesh()
    X, U = mesh["X"].numpy(), K.u_strain(mesh["X"]).numpy()
    conn, ne = mesh["conn"].numpy(), mesh["conn"].shape[0]
    per = [CF.tri3_energy(X, U, conn[e:e + 1], K.energy_mat(), K.ENERGY_W, K.energy_bk(), grads=False)[0] for e in range(ne)]
    assert min(per) > 0 and max(per) < 100 * min(per)
    whole = K.tri3_energy_expected(ne)[1]
    cuts = (0,) + K.ENERGY_RANGES + (ne,)
    assert len(set(cuts)) < len(cuts) and all(a <= b for a, b in zip(cuts, cuts[1:]))       # one empty range, all in order
    parts = [CF.tri3_energy(X, U, conn[a:b], K.energy_mat(), K.ENERGY_W, K.energy_bk())[0] for a, b in zip(cuts, cuts[1:]) if b > a]
    assert abs(sum(parts) - whole) <= K.LOSS_RTOL * whole
    n = K.ENERGY_N[-1]
    big = K.tri3_energy_expected(n)[1]
    assert abs(big - ((n // ne) * whole + sum(per[:n % ne]))) <= K.LOSS_RTOL * big
    # the sliced oracle sum against the exact (rational) sum of the per-element energies; the one-call serial sum drifts
    from fractions import Fraction
    exact = float(sum(Fraction(p) * int(k) for p, k in zip(per, np.bincount(np.arange(n) % ne, minlength=ne))))
    serial = CF.tri3_energy(X, U, K.repeated(mesh["conn"], n).numpy(), K.energy_mat(), K.ENERGY_W, K.energy_bk(), grads=False)[0]
    print(f"tri3 n={n}: sliced {abs(big - exact) / exact:.2e}, one call {abs(serial - exact) / exact:.2e} of the exact sum")
    assert abs(big - exact) <= 0.05 * K.LOSS_RTOL * exact and abs(serial - exact) > 0.3 * K.LOSS_RTOL * exact
    qm = K.quad_mesh()
    qc, nq, n4 = qm["conn"].numpy(), qm["conn"].shape[0], K.QUAD4_N[-1]
    per4 = [CF.quad4_energy(X, U, qc[e:e + 1], K.energy_mat(), grads=False)[0] for e in range(nq)]
    exact4 = float(sum(Fraction(p) * int(k) for p, k in zip(per4, np.bincount(np.arange(n4) % nq, minlength=nq))))
    assert min(per4) > 0 and abs(K.quad4_energy_expected(n4)[1] - exact4) <= 0.05 * K.LOSS_RTOL * exact4
    T = K.edge_tractions(n)
    assert (T > 0).all() and torch.unique(T[:, 0]).shape[0] == n
    edges, T257, loss, gX, gU = K.edge2_energy_expected(257)
    assert loss < 0 and np.abs(gX).max() > 0 and np.abs(gU).max() > 0
    # the table is read row by row: T alone differs from any constant row
    alt = -CF.edge2_energy(X, K.u_positive(X.shape[0]).numpy(), edges.numpy(), Tconst=T257[0].numpy())
    assert abs(alt - loss) > 1e-3 * abs(loss)
    C = R.plane_stress_C()
    xg, wg = R.triangle_gauss(4)
    assert abs(float(wg.sum()) - K.ENERGY_W) < 1e-15
    ref = R.domain_energy(mesh["X"], K.u_strain(mesh["X"]), mesh["conn"], C, xg, wg)
    nob = CF.tri3_energy(X, U, conn, K.energy_mat(), K.ENERGY_W, grads=False)[0]
    assert abs(ref.item() - nob) <= K.LOSS_RTOL * abs(nob) and abs(whole - nob) < 0.05 * nob


def test_post_statements():
    for kind in ("tri3", "quad4"):
        X, U, conn, g, vm = K.von_mises_base(kind)
        assert vm.min() > 0 and vm.max() < 100 * vm.min() and g.shape == (conn.shape[0], 2, 2)
        assert np.abs(K.von_mises_formula(g, 10e9, 0.3) / vm - 10e9 / K.POST_E).max() > 1e-3      # nu enters, not only E
    X, U, conn, g, vm = K.von_mises_base("tri3")
    g2 = CF.tri3_eval(X.numpy(), U.numpy(), conn.numpy(), np.full((conn.shape[0], 2), 1 / 3), np.arange(conn.shape[0]))[2]
    np.testing.assert_allclose(g2, g, rtol=K.POST_GRADU_RTOL, atol=K.POST_GRADU_ATOL)
    np.testing.assert_allclose(K.von_mises_formula(g2, K.POST_E, K.POST_NU), vm, rtol=K.VM_RTOL)
    for dim_u in (1, 2, 3):
        for n in (0, 1, 2, 257):
            grid, u, want = K.slopes_case(n, dim_u)
            assert grid.shape == (n,) and u.shape == (n, dim_u) and want.shape == (max(n - 1, 0), dim_u)
            if n >= 2:
                steps = grid[1:] - grid[:-1]
                assert (steps >= 0.5).all() and (n == 2 or steps.max() > 1.5 * steps.min())
                np.testing.assert_allclose(want.numpy(), K.slopes_by_autograd(grid, u).numpy(), rtol=K.SLOPE_RTOL, atol=K.SLOPE_ATOL)


def test_row_cases_are_permutations():
    for width in K.ROW_WIDTHS:
        for rows in K.row_counts(width)[:3]:
            src, idx = K.rows_case(rows, width, n_extra=rows // 3)
            assert src.shape == (rows, width) and idx.dtype == torch.int32
            assert torch.unique(idx).shape[0] == rows and (rows == 0 or (0 <= idx.min() and idx.max() < rows + rows // 3))


def test_adam_restatement_is_torch_adam():
    """``adam_rows_numpy`` with every row listed is ``torch.optim.Adam`` to the last bits, and the case has no cancelling
    entry: the relative bound of the GPU test is asked of numbers that carry all their digits."""
    c = K.adam_case()
    p = c["p"].clone().requires_grad_(True)
    opt = torch.optim.Adam([p], **{k if k != "beta1" else "betas": v if k != "beta1" else (K.ADAM_HYPER["beta1"], K.ADAM_HYPER["beta2"])
                                   for k, v in K.ADAM_HYPER.items() if k != "beta2"})
    pn, mn, vn = c["p"].numpy().copy(), np.zeros((K.ADAM_N, 2)), np.zeros((K.ADAM_N, 2))
    for k, g in enumerate(c["grads"]):
        p.grad = g.clone()
        opt.step()
        pn, mn, vn = K.adam_rows_numpy(pn, g.numpy(), mn, vn, np.arange(K.ADAM_N), k + 1, **K.ADAM_HYPER)
    st = opt.state[p]
    np.testing.assert_allclose(pn, p.detach().numpy(), rtol=4e-16)
    np.testing.assert_allclose(mn, st["exp_avg"].numpy(), rtol=4e-16)
    np.testing.assert_allclose(vn, st["exp_avg_sq"].numpy(), rtol=4e-16)
    rows = c["rows"].long()
    assert torch.unique(rows).shape[0] == K.ADAM_LISTED < K.ADAM_N and not rows.equal(rows.sort().values)
    assert (c["p"].abs() >= 0.5).all() and (c["v"] > 0).all()
    for g in c["grads"]:
        assert (torch.sign(g) == torch.sign(c["m"])).all() and (g.abs() >= 0.05).all()
