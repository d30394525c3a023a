"""The shifted Neo-Hookean tangent A(u) = c_K K_T(u) + c_M M on the device (the MASS instances of csrc/tri3_hyper_cg.hip and
csrc/quad4_hyper_cg.hip behind hfem_cg_setup_hyper_shifted) and the two Newton vector kernels of csrc/dynamics.hip, against
dense statements: K_T from tests/newton_reference.py / tests/quad4_newton_reference.py, M from tests/modal_reference.py.

Meshes and tile shapes are those of tests/test_gpu_newton.py and tests/test_gpu_quad4_newton.py.  Tolerances: their
``check_apply``'s, 1e-10 max|.| on q and on the diagonal blocks, p^T q within 1e-10 sum|p_i q_i| (rho = 2)."""
import ctypes as C

import numpy as np
import pytest
import torch

import hyper_reference as H
import modal_reference as MR
import newton_reference as N
import quad4_hyper_reference as Q
import quad4_newton_reference as QN
import test_gpu_newton as TN
import test_gpu_quad4_newton as TQ

F64 = torch.float64
pytestmark = pytest.mark.gpu
RHO = 2.0
COEFFS = [(1.0, 0.0), (0.0, 1.0), (0.3, 1.7)]
TRI_CASES = [("jittered", 0), ("plate", 64), ("jittered_x10", 4096)]     # one tile, many small tiles, default tiles + the loop
CASES = [("tri3",) + c for c in TRI_CASES] + [("quad4",) + c for c in TQ.CASES]
IDS = [f"{k}-{n}-{t}" for k, n, t in CASES]
_cache = {}


def mod(kind):
    return TQ if kind == "quad4" else TN


def field(kind, name):
    return H.field(mod(kind).mesh(name)[0])


def dense_K(kind, name, u, skip=None):
    coords, conn = mod(kind).mesh(name)[:2]
    if kind == "quad4":
        lam, mu = Q.lame()
        K = QN.dense_tangent(coords, u, conn, lam, mu, skip=skip)
    else:
        lam, mu = H.lame()
        K = N.dense_tangent(coords, u, conn, lam, mu, H.tri_W(), skip=skip)
    return N.restrict(K, mod(kind).free_mask(name))


def dense_M(kind, name, lumped):
    """rho M over the free rows in node order [2 n, 2 n]; computed once, never modified."""
    key = (kind, name, lumped)
    if key not in _cache:
        coords, conn = mod(kind).mesh(name)[:2]
        nodes = np.nonzero(mod(kind).free_mask(name).numpy())[0]
        _cache[key] = torch.from_numpy(MR.free_rows(MR.mass(coords.numpy(), conn.numpy(), rho=RHO, lumped=lumped), nodes))
    return _cache[key]


def make_solver(m, lf, mass="consistent", **kw):
    from hidenn_fem_amd.dynamics import HyperNewmarkSolver
    return HyperNewmarkSolver(m, lf, 1e-3, density=RHO, mass=mass, precond=kw.pop("precond", "block_jacobi"), **kw)


def lin_point(m):
    return m.u_free.detach().to(F64).contiguous()


def check_operator(kind, s, m, A, coeff, what):
    """``check_apply`` of the static tests on ``operator_apply``, and the blocks."""
    T = mod(kind)
    p = T.random_p(A.shape[0] // 2)
    q, pq = s.operator_apply(T.to_dev(m, p), coeff, u=lin_point(m))
    blocks = T.to_ref(m, s.diag)
    q = T.to_ref(m, q)
    want = (A @ p.reshape(-1)).reshape(-1, 2)
    eq = ((q - want).abs().max() / want.abs().max()).item()
    epq = abs(pq.item() - (p * want).sum().item()) / (p * want).abs().sum().item()
    wb = N.diag_blocks(A)
    eb = ((blocks - wb).abs().max() / wb.abs().max()).item()
    print(what, coeff, "q", f"{eq:.2e}", "p^T q", f"{epq:.2e}", "blocks", f"{eb:.2e}")
    assert eq <= 1e-10 and epq <= 1e-10 and eb <= 1e-10
    return p, q


# ---------------------------------------------------------------- 1. apply, p^T A p and blocks
@pytest.mark.parametrize("mass", ["consistent", "lumped"])
@pytest.mark.parametrize("kind,name,tile", CASES, ids=IDS)
def test_shifted_tangent_equals_the_dense_operator(kind, name, tile, mass):
    T = mod(kind)
    u = field(kind, name)
    m = T.make_model(name, u)
    lf = T.make_loss(tile_elems=tile)
    s = make_solver(m, lf, mass)
    K, M = dense_K(kind, name, u), dense_M(kind, name, mass == "lumped")
    for c_k, c_m in COEFFS:
        p, q = check_operator(kind, s, m, c_k * K + c_m * M, (c_k, c_m), f"{kind} {name}-{tile} {mass}")
        assert s.info[1].item() == 0
        if (c_k, c_m) == (1.0, 0.0):                                   # the plain solver's apply, to the same bound
            q0, _ = T.make_solver(m, lf).apply(T.to_dev(m, p))
            q0 = T.to_ref(m, q0)
            assert ((q - q0).abs().max() / q0.abs().max()).item() <= 1e-10
    # hfem_cg_setup_hyper on the same handle: plain K_T again
    T.check_apply(s.newton, m, K, f"{kind} {name}-{tile} back to plain")


# ---------------------------------------------------------------- 2. one inverted element
@pytest.mark.parametrize("mass", ["consistent", "lumped"])
@pytest.mark.parametrize("kind,name,tile", [("tri3", "jittered", 0), ("tri3", "plate", 64), ("quad4", "jittered", 0),
                                            ("quad4", "plate", 64)])
def test_inverted_element_keeps_its_mass_and_loses_its_stiffness(kind, name, tile, mass):
    T = mod(kind)
    coords, conn = T.mesh(name)[:2]
    if kind == "quad4":
        v, _ = Q.invert_one_cell(coords, field(kind, name), conn)
        t = Q.element_terms(coords, v, conn, *Q.lame())
    else:
        v, _ = H.invert_one_element(coords, field(kind, name), conn)
        t = H.element_terms(coords, v, conn, *H.lame(), H.tri_W())
    assert int(t["inverted"].sum()) == 1
    K, M = dense_K(kind, name, v, skip=t["inverted"]), dense_M(kind, name, mass == "lumped")
    m = T.make_model(name, v)
    s = make_solver(m, T.make_loss(tile_elems=tile), mass)
    for c_k, c_m in COEFFS[1:]:
        check_operator(kind, s, m, c_k * K + c_m * M, (c_k, c_m), f"{kind} {name} inverted {mass}")
        assert s.info[1].item() == 1.0 and abs(s.info[0].item() - t["J"].min().item()) <= 1e-13


# ---------------------------------------------------------------- 2b. the QUAD4 apply that recomputes c_q (STORED = false)
RECOMPUTE = ("recompute", "HFEM_QUAD4_TANGENT_RECOMPUTE")


def _recompute_cases():
    """What the child process runs: every QUAD4 case of 1. and 2. on the library that is already loaded."""
    for _, name, tile in [c for c in CASES if c[0] == "quad4"]:
        for mass in ("consistent", "lumped"):
            test_shifted_tangent_equals_the_dense_operator("quad4", name, tile, mass)
    for name, tile in (("jittered", 0), ("plate", 64)):
        for mass in ("consistent", "lumped"):
            test_inverted_element_keeps_its_mass_and_loses_its_stiffness("quad4", name, tile, mass)


def test_quad4_cases_on_the_build_that_recomputes_the_stored_coefficients():
    """The product library launches ``quad4_hyper_cg_apply_kernel<..., STORED = true, MASS>``; the other ``STORED`` path is the
    A/B build ``build.py --tag recompute --define HFEM_QUAD4_TANGENT_RECOMPUTE``.  A fresh child process loads that library
    (a process holds one) and runs the QUAD4 cases of 1. and 2. on it, same bounds."""
    import os
    import subprocess
    import sys
    from hidenn_fem_amd.csrc import build
    tag, define = RECOMPUTE
    lib = os.path.join(build.HERE, f"libhidenn_hip_{tag}.so")
    deps = [os.path.join(build.HERE, s) for s in build.SOURCES] + [h if os.path.isabs(h) else os.path.join(build.HERE, h)
                                                                   for h in build.HEADERS]
    if build._stale(lib, deps):                              # a checkout's build() has made it; otherwise make it now
        lib = build.build(tag=tag, defines=[define])
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; from hidenn_fem_amd import _lib; _lib.LIB_PATH = %r; "
            "import test_gpu_hyper_dynamics_kernels as K; K._recompute_cases(); print('recompute cases ok')"
            % (build.ROOT, here, lib))
    r = subprocess.run([sys.executable, "-c", code], cwd=here, capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "recompute cases ok" in r.stdout


# ---------------------------------------------------------------- 3. iteration mode against the standalone apply
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_one_graph_of_iterations_equals_pcg_composed_on_operator_apply(kind):
    """``test_one_graph_of_iterations_equals_pcg_composed_on_apply`` of the static tests on A = 0.3 K_T + 1.7 rho M (positive
    definite: asserted on the host-composed recursion): one captured graph of five iterations against five PCG iterations
    composed on the host from ``operator_apply`` and the blocks, 1e-10."""
    from hidenn_fem_amd import _lib
    T = mod(kind)
    coeff = COEFFS[2]
    m = T.make_model("plate", 0.3 * field(kind, "plate"))
    s = make_solver(m, T.make_loss(), iters_per_graph=5)
    nw, u = s.newton, lin_point(m)
    g = T.to_dev(m, T.random_p(s.n_u, seed=13))
    s.operator_apply(g, coeff, u=u)
    dinv, pd = N.jacobi_inverse(s.diag.cpu())
    assert pd.all()
    dinv = dinv.to(T.dev())
    d, r = torch.zeros_like(g), -g.clone()
    z = N.apply_blocks(dinv, r)
    rho, p, beta = (r * z).sum(), torch.zeros_like(g), 0.0
    for _ in range(5):
        p = z + beta * p
        q, pq = s.operator_apply(p.contiguous(), coeff, u=u)
        assert pq.item() > 0
        alpha = rho / pq
        d, r = d + alpha * p, r - alpha * q
        z = N.apply_blocks(dinv, r)
        rho_new = (r * z).sum()
        beta, rho = rho_new / rho, rho_new
    nw._g.copy_(g)
    nw._delta.zero_()
    _lib.check(_lib.lib().hfem_cg_start(nw._h, nw._g.data_ptr(), nw._g.data_ptr(), 1e-30, 0.0, 1000, _lib.stream_ptr(T.dev())),
               "hfem_cg_start")
    torch.cuda.synchronize()
    nw._replay()
    st = nw._read_status()
    err = ((nw._delta - d).abs().max() / d.abs().max()).item()
    print(kind, "iterations", st[0], "delta", f"{err:.2e}", "|r|", st[1], r.norm().item())
    assert st[0] == 5.0 and st[10] == 0.0
    assert err <= 1e-10 and abs(st[1] - r.norm().item()) <= 1e-10 * g.norm().item()


# ---------------------------------------------------------------- 4. argument errors leave the handle as it was
@pytest.mark.parametrize("kind", ["tri3", "quad4"])
def test_argument_errors_leave_the_handle_as_it_was(kind):
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.dynamics import NewmarkSolver
    import test_gpu_modal as TM
    lib, err = _lib.lib(), _lib.lib().hfem_last_error
    T = mod(kind)
    u = field(kind, "plate")
    m = T.make_model("plate", u)
    s = make_solver(m, T.make_loss())
    A = 0.3 * dense_K(kind, "plate", u) + 1.7 * dense_M(kind, "plate", False)
    p = T.to_dev(m, T.random_p(s.n_u))
    s.operator_apply(p, COEFFS[2], u=lin_point(m))
    nw, st = s.newton, _lib.stream_ptr(T.dev())
    lame, W = nw._lame, float(nw.loss_fn._W)

    def setup(h=None, c_k=0.3, c_m=1.7, ufix=True):
        return lib.hfem_cg_setup_hyper_shifted(nw._h if h is None else h, nw._xf.data_ptr(), nw._xfix.data_ptr(), nw._u.data_ptr(),
                                               nw._ufix.data_ptr() if ufix else None, lame, W, c_k, c_m * RHO, 0, 1, None, None, st)

    def still_bound():
        q = torch.empty_like(p)
        pq = torch.empty((), dtype=F64, device=T.dev())
        _lib.check(lib.hfem_cg_apply(nw._h, p.data_ptr(), q.data_ptr(), pq.data_ptr(), st), "hfem_cg_apply")
        want = (A @ T.to_ref(m, p).reshape(-1)).reshape(-1, 2)
        assert ((T.to_ref(m, q) - want).abs().max() / want.abs().max()).item() <= 1e-10

    for kw in (dict(c_k=-0.1), dict(c_m=-1.0), dict(c_k=float("nan")), dict(c_m=float("inf")), dict(c_k=0.0, c_m=0.0)):
        assert setup(**kw) < 0 and b"c_k and c_m" in err(), kw
        still_bound()
    assert setup(ufix=False) < 0 and b"hfem_cg_setup_hyper_shifted: the plan reads Dirichlet rows: u_fixed must be given" in err()
    still_bound()
    lin = NewmarkSolver(TM.make_model(kind), TM.make_loss("physical"), 1e-3, precond="none")      # a handle of hfem_cg_create
    pl = T.random_p(lin.n_u).to(T.dev())
    before, _ = lin.operator_apply(pl)
    assert setup(h=lin._h) < 0 and b"hfem_cg_setup_hyper_shifted: this solver was created by hfem_cg_create" in err()
    still_bound()
    after = torch.empty_like(pl)                             # the refused handle too: still bound to its own c_K K + c_M M
    pq = torch.empty((), dtype=F64, device=T.dev())
    _lib.check(lib.hfem_cg_apply(lin._h, pl.data_ptr(), after.data_ptr(), pq.data_ptr(), st), "hfem_cg_apply")
    assert ((after - before).abs().max() / before.abs().max()).item() <= 1e-10
    # the existing entry point's messages still carry its own name
    assert lib.hfem_cg_setup_hyper(lin._h, nw._xf.data_ptr(), nw._xfix.data_ptr(), nw._u.data_ptr(), nw._ufix.data_ptr(), lame, W, 1,
                                   None, None, st) < 0 and b"hfem_cg_setup_hyper: this solver was created by hfem_cg_create" in err()


# ---------------------------------------------------------------- 5. the vector kernels
LENGTHS = [1, 63, 64, 65, 256 * 1024 + 1]                    # one row; wave edges; past the grid cap


def _ulp_tol(*terms):
    return 4.0 * np.spacing(np.max(np.abs(np.stack([np.asarray(t, dtype=np.float64) for t in terms])), axis=0))


@pytest.mark.parametrize("n", LENGTHS)
def test_vector_kernels_against_the_formulas(n):
    """Against numpy.longdouble: 4 ulp of the largest term of every entry, bit-identical on a repeat, M v~ = NULL is alpha_R = 0."""
    from hidenn_fem_amd import _lib
    lib, dev = _lib.lib(), torch.device("cuda:0")
    rng = np.random.default_rng(n)
    s_len, c_k, c_m, alpha_r, load = 0.37, 2.3e-4, 1.013, 0.21, -1.7
    host = {k: rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-3, 4) for k in ("a", "d", "ut", "ma", "md", "mv", "f", "b")}
    d = {k: torch.from_numpy(x).to(dev) for k, x in host.items()}
    ld = {k: x.astype(np.longdouble) for k, x in host.items()}
    L = np.longdouble
    ptr = lambda t: None if t is None else t.data_ptr()
    new = lambda: torch.full((n, 2), float("nan"), dtype=F64, device=dev)

    def trial(in_place=False):
        a_t, u_t, ma_t = (d["a"].clone(), new(), d["ma"].clone()) if in_place else (new(), new(), new())
        src = (a_t, ma_t) if in_place else (d["a"], d["ma"])
        _lib.check(lib.hfem_newmark_trial(0, ptr(src[0]), ptr(d["d"]), ptr(d["ut"]), ptr(src[1]), ptr(d["md"]), 2 * n, s_len, c_k,
                                          ptr(a_t), ptr(u_t), ptr(ma_t), None), "trial")
        return a_t, u_t, ma_t

    a_t, u_t, ma_t = trial()
    at_ref = ld["a"] + L(s_len) * ld["d"]
    t_a = (host["a"], s_len * host["d"])
    checks = ((a_t, at_ref, t_a, "a_t"), (u_t, ld["ut"] + L(c_k) * at_ref, (host["ut"],) + tuple(c_k * t for t in t_a), "u_t"),
              (ma_t, ld["ma"] + L(s_len) * ld["md"], (host["ma"], s_len * host["md"]), "(M a)_t"))
    for got, ref, terms, what in checks:
        e = np.abs(got.cpu().numpy() - ref.astype(np.float64))
        assert (e <= _ulp_tol(*terms)).all(), (what, n, e.max())
    assert all(torch.equal(x, y) for x, y in zip((a_t, u_t, ma_t), trial()))
    assert all(torch.equal(x, y) for x, y in zip((a_t, u_t, ma_t), trial(in_place=True)))

    def residual(mv, alpha, neg=True):
        r, nr = new(), new() if neg else None
        _lib.check(lib.hfem_newmark_residual(0, ptr(d["ma"]), ptr(mv), ptr(d["f"]), ptr(d["b"]), 2 * n, c_m, alpha, load, ptr(r),
                                             ptr(nr), None), "residual")
        return r, nr

    r, nr = residual(d["mv"], alpha_r)
    r_ref = L(c_m) * ld["ma"] + L(alpha_r) * ld["mv"] + ld["f"] - L(load) * ld["b"]
    t_r = (c_m * host["ma"], alpha_r * host["mv"], host["f"], load * host["b"])
    assert (np.abs(r.cpu().numpy() - r_ref.astype(np.float64)) <= _ulp_tol(*t_r)).all()
    assert torch.equal(nr, -r)
    r2, nr2 = residual(d["mv"], alpha_r)
    assert torch.equal(r, r2) and torch.equal(nr, nr2)
    assert torch.equal(residual(d["mv"], alpha_r, neg=False)[0], r)
    r0, _ = residual(None, alpha_r)                            # M v~ = NULL is alpha_R = 0
    r1, _ = residual(d["mv"], 0.0)
    assert torch.equal(r0, r1)
    r0_ref = L(c_m) * ld["ma"] + ld["f"] - L(load) * ld["b"]
    assert (np.abs(r0.cpu().numpy() - r0_ref.astype(np.float64)) <= _ulp_tol(t_r[0], t_r[2], t_r[3])).all()
    torch.cuda.synchronize()
