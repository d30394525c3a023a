"""QUAD4 kernels off the default tile shape and off structured numbering.

Every other QUAD4 test runs `structured_quad_mesh` at the planner's default tile: one kernel instance, 4-valent nodes, cells
counter-clockwise from the same corner.  Here the tile shape is chosen so that each product instance runs with real work
(`tile_elems` 600 and 800, `store_policy` 2, `quad4_const_caps` 0), and the mesh is also the Delaunay mesh split into quads
(`tests/quad_meshes.py`: valence 1..11) in a random numbering with rotated and reversed cells.  The reference is always
`oracle.quad4` autograd minus `oracle.ref_chain.edge_energy` in fp64 on the CPU, at the tolerances `tests/test_quad4.py` holds
QUAD4 to: loss 1e-12 relative, gradients 1e-10 max|g|.

The library cannot be asked which instance it launched, so `quad4_energy_branch` / `quad4_cg_apply_branch` restate the
dispatch of `hfem_quad4_energy_plan_ex` (csrc/quad4.hip) and `launch_quad4_cg_apply` (csrc/quad4_cg.hip) from the plan's
statistics; the intended branch is asserted on host-only plans (CPU test) and again on the device plan of every GPU case.

Which test reaches which product instance (S = structured 61 x 45, T = split Delaunay, number = `tile_elems`):

* `quad4_energy_fast_kernel`
  - `<256,3,3,0,560,false,672>` (const caps): every older QUAD4 test; here `test_energy_per_branch[S0]`, `[T0]`, numbering at 0.
  - `<256,3,3,0,560,false,672,double2,false,2>` (const caps, nt stores): `test_quad4.py`, the 10^6-cell test only.
  - `<256,3,3,0>` (runtime strides): `test_energy_per_branch[S600]` and `[S0-nocaps]`.
  - `<256,4,4,0>`: `test_energy_per_branch[S800]`, `[T800]`, the numbering tests at 800; slot 3 populated.
  - `<256,4,4,0,0,false,0,double2,false,2>` (generic nt): `test_energy_per_branch[S800-nt]`, `[T800-nt]`.
  - `<256,4,4,0,0,HASB,0,V2,PHYS>` for body force, physical convention, fp32 rows (7 instances): `test_quad4.py` with slot 3
    idle; `test_feature_instances_with_slot_3_populated[S]`, `[T]` with tiles of more than 768 nodes and slots.
  - `<256,4,4,0,560>` (compile-time accumulator stride, runtime node stride): NOT REACHED BY ANY TEST.  It needs a tile of
    at most 716 nodes with more than 768 element slots; a planar quad mesh has about as many nodes as cells, and no host
    plan of S or T at `tile_elems` 16..4096 (step 8) with `plan_node_cap` -1, 0, 600, 650, 700, 716 gets there.
* `quad4_cg_apply_kernel`
  - `<256,3,3,PHYS>`: `test_gpu_solve_quad4.py`; here `test_cg_apply_and_block_jacobi_per_branch[S600-*]`, `[T0-*]`.
  - `<256,4,4,PHYS>`: `test_cg_apply_and_block_jacobi_per_branch[S800-*]`, `[T800-*]` only.
* `quad4_cg_diag_kernel<256,4,4,PHYS>` (the only instance): `test_gpu_solve_quad4.py` with slot 3 idle;
  `test_cg_apply_and_block_jacobi_per_branch[S800-*]`, `[T800-*]` with it populated.

The reference gradient convention (`dN_dx = Jinv * dN_dxi`) is not invariant to a cell's local node order (TRI3:
`test_gpu_properties.py::test_invariance_to_element_order_and_node_renumbering` part 3): rotating a cell's corners or reversing
it changes the reference-convention energy by 1e-3 relative on these meshes, in the oracle as in the kernels.  So every
numbering is compared with the oracle of the renumbered mesh in both conventions, and with the un-renumbered run in the
physical convention (invariant to all of it) and, for the cell and node permutations alone, in the reference convention."""
import contextlib
import copy
import functools
import math

import numpy as np
import pytest
import torch

import quad_meshes as QM
from conftest import b_force_fn

F64 = torch.float64
CONVS = ["reference", "physical"]


# ---------------------------------------------------------------- meshes (built once, never written to)
@functools.lru_cache(maxsize=None)
def _mesh(name):
    """"S", "T", or "<S|T>:<orient>[:plain]" = renumbered with seed 11 (plain: cells and nodes permuted only).  Returns
    (mesh6, old_of_new or None)."""
    from hidenn_fem_amd.mesh import structured_quad_mesh
    if name == "S":
        return structured_quad_mesh(61, 45, jitter=0.25, seed=4, dtype=F64), None
    if name == "T":
        return QM.split_tri_quads(), None
    base, orient, *plain = name.split(":")
    return QM.renumber(_mesh(base)[0], seed=11, rotate=not plain, orient=orient)


@functools.lru_cache(maxsize=None)
def _u_field(base):
    """One nodal field per base mesh, by ORIGINAL node id: 50 times the model's own initial scale (1e-5), as the other QUAD4
    tests scale `u_free`."""
    n = _mesh(base)[0][0].shape[0]
    return 50.0 * 1e-5 * torch.randn(n, 2, dtype=F64, generator=torch.Generator().manual_seed(1))


def _u_caller(name, u_mask):
    """The field of `_u_field` on the free rows of mesh `name`, in the caller's row order."""
    mesh, old = _mesh(name)
    u = _u_field(name.split(":")[0])
    u = u if old is None else u[old]
    return u[u_mask]


def _masks(mesh, x_fixed):
    geom, bc = mesh[2], mesh[3]
    return (geom if x_fixed == "geom" else bc), bc


# ---------------------------------------------------------------- the dispatch, restated
def quad4_energy_branch(stats, const_caps=True, fp32=False, phys=False, hasb=False):
    """Which `quad4_energy_fast_kernel` instance `hfem_quad4_energy_plan_ex` launches (product build, not deterministic)."""
    n, o, e, nt = stats["max_tile_nodes"], stats["max_tile_owned"], stats["max_tile_elems"], stats["store_policy"] == 2
    assert n <= 4 * 256 and e <= 4 * 256                         # what the entry point accepts at all
    if fp32 or phys or hasb:
        return "feature<4,4>"
    default_shape = const_caps and n <= 672 and o <= 560 and e <= 3 * 256
    if nt:
        return "const_caps_nt" if default_shape else "generic_nt<4,4>"
    if default_shape:
        return "const_caps"
    if n <= 3 * 256 and e <= 3 * 256:
        return "<3,3,0>"
    if const_caps and o <= 560 and n * 32 + 560 * 32 + 128 <= 40960:
        return "<4,4,0,560>"
    return "<4,4,0>"


def quad4_cg_apply_branch(stats):
    return "<3,3>" if stats["max_tile_nodes"] <= 3 * 256 and stats["max_tile_elems"] <= 3 * 256 else "<4,4>"


def _slot3_populated(stats):
    return stats["max_tile_nodes"] > 768 and stats["max_tile_elems"] > 768


# id -> (mesh, tile_elems, options, energy branch, CG apply branch, slot 3 populated)
CASES = {
    "S0": ("S", 0, {}, "const_caps", "<3,3>", False),
    "S600": ("S", 600, {}, "<3,3,0>", "<3,3>", False),
    "S800": ("S", 800, {}, "<4,4,0>", "<4,4>", True),
    "T0": ("T", 0, {}, "const_caps", "<3,3>", False),
    "T800": ("T", 800, {}, "<4,4,0>", "<4,4>", True),
    "S800-nt": ("S", 800, {"store_policy": 2}, "generic_nt<4,4>", "<4,4>", True),
    "T800-nt": ("T", 800, {"store_policy": 2}, "generic_nt<4,4>", "<4,4>", True),
    "S0-nocaps": ("S", 0, {"quad4_const_caps": 0}, "<3,3,0>", "<3,3>", False),
}


@contextlib.contextmanager
def _options(**opts):
    from hidenn_fem_amd import _lib
    L = _lib.lib()
    prev = {}
    try:
        for k, v in opts.items():
            prev[k] = L.hfem_get_option(k.encode())
            _lib.check(L.hfem_set_option(k.encode(), v), "hfem_set_option")
        yield
    finally:
        for k, v in prev.items():
            L.hfem_set_option(k.encode(), v)


def _const_caps():
    from hidenn_fem_amd import _lib
    return bool(_lib.lib().hfem_get_option(b"quad4_const_caps"))


def _assert_case(stats, case):
    _, _, opts, want_energy, want_cg, slot3 = CASES[case]
    assert quad4_energy_branch(stats, _const_caps()) == want_energy, (case, stats)
    assert quad4_cg_apply_branch(stats) == want_cg, (case, stats)
    assert _slot3_populated(stats) == slot3, (case, stats)
    if "store_policy" in opts:
        assert stats["store_policy"] == 2


def _new_model(name, device=None, dtype=F64, conv="reference", reorder="auto", x_fixed="geom"):
    """A fresh model of mesh `name` carrying `_u_field`; `x_fixed`: which nodes have fixed coordinates ("geom": the
    geometric boundary, "bc": the Dirichlet nodes only)."""
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D, QuadShapeNN2D
    mesh, _ = _mesh(name)
    nc, conn, geom, bc, mn, edges = mesh
    xmask, umask = _masks(mesh, x_fixed)
    torch.manual_seed(0)
    m = PiecewiseLinearShapeNN2D(nc.to(dtype), conn, boundary_mask=xmask, dirichlet_mask=umask, u_fixed=0.0,
                                 neumann_edges=edges, reorder=reorder)
    assert isinstance(m, QuadShapeNN2D)
    m.grad_convention = conv
    if device is not None:
        m = m.to(device)
    with torch.no_grad():
        m.u_free.copy_(m.from_caller_order(_u_caller(name, ~umask).to(m.u_free.device, dtype), "u"))
    return m


# ================================================================ CPU: the helper module and the branch table
def test_split_and_renumbered_meshes_are_valid_and_the_oracle_energy_does_not_change():
    from oracle import quad4 as Q, ref_chain as R
    from test_radapt_quad4_host import quad4_measure_np
    (nc, conn, geom, bc, mn, edges), _ = _mesh("T")
    X, cn = nc.numpy(), conn.numpy()
    q, r, inv = quad4_measure_np(X[cn], X[cn])
    assert inv.sum() == 0 and q.min() > 0.1 and (r == 1.0).all()         # convex, counter-clockwise (q > 0 at all 4 corners)
    assert cn.shape == (4137, 4) and X.shape == (4312, 2)
    assert np.unique(cn).size == X.shape[0] and (np.sort(cn, axis=1)[:, 1:] != np.sort(cn, axis=1)[:, :-1]).all()
    val = QM.valence(cn, X.shape[0])
    hist = np.bincount(val)
    assert hist[:4].sum() > 0 and hist[6:].sum() > 0 and val.min() == 1 and val.max() == 11, hist
    # masks: a midpoint inherits a flag iff both ends of its edge carry it; every Neumann edge was split in two
    assert int(geom.sum()) > int(bc.sum()) > 0 and edges.shape[0] % 2 == 0 and edges.shape[0] > 0
    assert mn[edges].all() and geom[edges].all()
    em = X[edges.numpy()]
    assert np.allclose(em[0::2, 1], em[1::2, 0]) and np.abs(em[0::2, 0] + em[1::2, 1] - 2 * em[0::2, 1]).max() < 1e-15

    def energy(mesh, U, conv, with_edges=True):
        c, k, *_, e = mesh
        out = Q.quad4_domain_energy(c, U, k, R.plane_stress_C(), None, conv)
        return (out - R.edge_energy(c, U, e, *R.interval_gauss(2))).item() if with_edges else out.item()

    def signed_area2(mesh):
        P = mesh[0].numpy()[mesh[1].numpy()]
        d1, d2 = P[:, 2] - P[:, 0], P[:, 3] - P[:, 1]
        return d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]

    for base in ("S", "T"):
        mesh0, U0 = _mesh(base)[0], _u_field(base)
        c0, k0 = mesh0[0].numpy(), mesh0[1].numpy()
        q0 = quad4_measure_np(c0[k0], c0[k0])[0].min()
        for conv in CONVS:
            e0 = energy(mesh0, U0, conv)
            for orient in ("ccw", "cw", "mixed"):
                for plain in (False, True):
                    mesh1, old = _mesh(f"{base}:{orient}" + (":plain" if plain else ""))
                    c1, k1 = mesh1[0].numpy(), mesh1[1].numpy()
                    q1, _, inv1 = quad4_measure_np(c1[k1], c1[k1])             # valid against its own orientation
                    assert inv1.sum() == 0 and abs(q1.min() - q0) < 1e-12
                    assert torch.equal(mesh1[0], mesh0[0][old]) and torch.equal(mesh1[2], mesh0[2][old])
                    assert sorted(QM.valence(k1, c1.shape[0])) == sorted(QM.valence(k0, c1.shape[0]))
                    e1 = energy(mesh1, U0[old], conv)
                    if conv == "physical" or (plain and orient == "ccw"):
                        assert abs(e1 - e0) <= 1e-13 * abs(e0), (base, conv, orient, plain)
                    else:                                       # the reference convention sees a cell's local node order (F4)
                        assert abs(e1 - e0) > 1e-6 * abs(e0), (base, conv, orient, plain)
    # orientation as asked for
    assert (signed_area2(_mesh("T:ccw")[0]) > 0).all() and (signed_area2(_mesh("T:cw")[0]) < 0).all()
    assert int((signed_area2(_mesh("T:mixed")[0]) < 0).sum()) == 4137 // 2


@pytest.mark.parametrize("case", list(CASES))
def test_host_plans_land_in_the_intended_branch(case):
    from hidenn_fem_amd.plan import TilePlan
    name, te, opts, *_ = CASES[case]
    m = _new_model(name)
    with _options(**opts):
        p = TilePlan(m.connectivity, m.Nnodes, coords_hint=m.initial_node_coords, x_src=m._x_src, u_src=m._u_src,
                     edges=m.neumann_edges, tile_elems=te, device=None, nodes_per_elem=4)
        try:
            _assert_case(p.stats, case)
            assert p.stats["lds_bytes"] <= 64 * 1024
        finally:
            p.close()
    assert _const_caps()                                             # restored


# ================================================================ GPU
def _dev():
    return torch.device("cuda:0")


def _lf(dtype=F64, **kw):
    from hidenn_fem_amd.loss import EnergyLoss2D
    return EnergyLoss2D(device=_dev(), dtype=dtype, **kw)


def _bf_gpu(x):
    return b_force_fn(x.cpu().double()).to(x.device)


_REF = {}


def _oracle(name, conv="reference", hasb=False, x_fixed="geom", with_edges=True, u=None):
    """(loss, dE/dx_free, dE/du_free) of mesh `name` at its own coordinates and `_u_field` (or the caller-order rows `u`), rows
    in the caller's order.  Computed once per key and shared."""
    from oracle import quad4 as Q, ref_chain as R
    key = (name, conv, hasb, x_fixed, with_edges)
    if u is None and key in _REF:
        return _REF[key]
    mesh, _ = _mesh(name)
    nc, conn, geom, bc, mn, edges = mesh
    xmask, umask = _masks(mesh, x_fixed)
    xf = nc[~xmask].clone().requires_grad_(True)
    uf = (_u_caller(name, ~umask) if u is None else u).clone().requires_grad_(True)
    X = R.assemble_coords(nc.shape[0], ~xmask, xf, xmask, nc[xmask])
    U = R.assemble_u(nc.shape[0], ~umask, uf, umask, torch.tensor(0.0, dtype=F64))
    e = Q.quad4_domain_energy(X, U, conn, R.plane_stress_C(), b_force_fn if hasb else None, conv)
    if with_edges:
        e = e - R.edge_energy(X, U, edges, *R.interval_gauss(2))
    e.backward()
    out = (e.item(), xf.grad, uf.grad)
    if u is None:
        _REF[key] = out
    return out


def _grads(m):
    return (m.to_caller_order(m.node_coords_free.grad, "x").detach().cpu().double(),
            m.to_caller_order(m.u_free.grad, "u").detach().cpu().double())


def _run(lf, m, bf=None):
    m.zero_grad(set_to_none=True)
    loss = lf(m, b_force=bf)
    loss.backward()
    return (loss.item(),) + _grads(m)


def _assert_close(got, want, what):
    """The suite's QUAD4 tolerances against the autograd oracle: loss 1e-12 relative, gradients 1e-10 max|g|."""
    (e, gx, gu), (e_ref, gx_ref, gu_ref) = got, want
    de = abs(e - e_ref) / abs(e_ref)
    dx = (gx - gx_ref).abs().max().item() / gx_ref.abs().max().item()
    du = (gu - gu_ref).abs().max().item() / gu_ref.abs().max().item()
    print(f"{what}: loss {de:.3e}, gx {dx:.3e}, gu {du:.3e}")
    assert de <= 1e-12, (what, e, e_ref)
    assert dx <= 1e-10, what
    assert du <= 1e-10, what


# ---------------------------------------------------------------- a. energy and gradients per branch
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_energy_per_branch(case):
    name, te, opts, *_ = CASES[case]
    ref = _oracle(name)
    with _options(**opts):                                           # quad4_const_caps is read at every launch
        m = _new_model(name, _dev())                                 # a fresh model: plans are cached per (device, tile_elems)
        lf = _lf(tile_elems=te)
        _assert_case(m.tile_plan(te).stats, case)
        got = _run(lf, m)
        _assert_close(got, ref, f"{case} backward()")
        with torch.no_grad():                                        # the autograd-free form overwrites .grad
            for p_ in m.parameters():
                p_.grad.fill_(3.0)
        e_d = lf.value_and_grad_(m).item()
        _assert_close((e_d,) + _grads(m), ref, f"{case} value_and_grad_")
        lf.quad4_planless = True                                     # global fp64 atomics: no plan, no tile shape
        planless = _run(lf, m)
        lf.quad4_planless = False
        _assert_close(planless, ref, f"{case} planless")
        _assert_close(got, planless, f"{case} tiled vs planless")


# ---------------------------------------------------------------- b. feature instances with slot 3 populated
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "T"])
def test_feature_instances_with_slot_3_populated(name):
    """{reference, physical} x {no body force, b_force_fn} x {fp64, fp32 rows} at tile_elems 800: the general <4,4> instances
    with local nodes and element slots 768.. in use.  fp32 rows by the rule of
    test_quad4.py::test_quad4_fp32_rows_physical_convention_and_deterministic_instances."""
    te = 800
    m = _new_model(name, _dev())
    st = m.tile_plan(te).stats
    assert _slot3_populated(st), st
    for conv in CONVS:
        for hasb in (False, True):
            want = "<4,4,0>" if (conv, hasb) == ("reference", False) else "feature<4,4>"
            assert quad4_energy_branch(st, _const_caps(), phys=conv == "physical", hasb=hasb) == want
            lf = _lf(tile_elems=te, grad_convention=conv)
            _assert_close(_run(lf, m, _bf_gpu if hasb else None), _oracle(name, conv, hasb), f"{name} {conv} body={hasb}")
    m32 = _new_model(name, _dev(), dtype=torch.float32)
    m64 = copy.deepcopy(m32).double()
    st32 = m32.tile_plan(te).stats
    assert _slot3_populated(st32) and quad4_energy_branch(st32, _const_caps(), fp32=True) == "feature<4,4>"
    for conv in CONVS:
        for hasb in (False, True):
            lf32 = _lf(torch.float32, tile_elems=te, grad_convention=conv)
            lf64 = _lf(tile_elems=te, grad_convention=conv)
            lf64._mat, lf64._W, lf64._ci, lf64._cj = lf32._mat, lf32._W, lf32._ci, lf32._cj   # the fp32 object's rounded constants
            bf = _bf_gpu if hasb else None
            l32, gx32, gu32 = _run(lf32, m32, bf)
            l64, gx64, gu64 = _run(lf64, m64, bf)
            assert m32.u_free.grad.dtype == torch.float32
            print(f"{name} fp32 rows {conv} body={hasb}: loss {abs(l32 - l64) / abs(l64):.3e}")
            assert abs(l32 - l64) <= 2e-7 * abs(l64)
            for a, b in ((gx32, gx64), (gu32, gu64)):
                want = b.float().double()
                ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(1e-30)
                assert ((a - want).abs() <= 1.01 * ulp).all(), (conv, hasb)


# ---------------------------------------------------------------- c. numbering
_BASE_RUN = {}


def _full(name, g, mask):
    """Caller-order free rows -> [Nn, 2] by ORIGINAL node id (fixed rows 0)."""
    mesh, old = _mesh(name)
    out = torch.zeros(mesh[0].shape[0], 2, dtype=F64)
    out[~mask] = g
    if old is None:
        return out
    back = torch.empty_like(out)
    back[old] = out
    return back


def _run_full(name, te, conv):
    mesh, _ = _mesh(name)
    m = _new_model(name, _dev())
    st = m.tile_plan(te).stats
    e, gx, gu = _run(_lf(tile_elems=te, grad_convention=conv), m)
    return (e, gx, gu), (e, _full(name, gx, mesh[2]), _full(name, gu, mesh[3])), st


def _base_run(base, te, conv):
    key = (base, te, conv)
    if key not in _BASE_RUN:
        _BASE_RUN[key] = _run_full(base, te, conv)[1]
    return _BASE_RUN[key]


@pytest.mark.gpu
@pytest.mark.parametrize("orient", ["ccw", "cw", "mixed"])
@pytest.mark.parametrize("te", [0, 800])
@pytest.mark.parametrize("base", ["S", "T"])
def test_numbering_cell_order_node_ids_corner_rotation_and_orientation(base, te, orient):
    """Cells permuted, nodes renumbered, corners rotated, cells reversed: against the oracle of the renumbered mesh (both
    conventions) and against the run on the mesh as generated, brought back through the inverse node map, at the bound of
    test_gpu_properties.py::test_invariance_to_element_order_and_node_renumbering (loss 1e-12, gradients 1e-10 max|g|) --
    in the physical convention, and in the reference convention for the permutations alone (module docstring)."""
    pairs = [(f"{base}:{orient}", conv) for conv in CONVS]
    if orient == "ccw":
        pairs.append((f"{base}:ccw:plain", "reference"))
    for name, conv in pairs:
        got, got_full, st = _run_full(name, te, conv)
        assert _slot3_populated(st) == (te == 800) and quad4_energy_branch(st, _const_caps()) == ("<4,4,0>" if te else "const_caps")
        _assert_close(got, _oracle(name, conv), f"{name} te={te} {conv} vs oracle")
        if conv == "physical" or name.endswith(":plain"):
            _assert_close(got_full, _base_run(base, te, conv), f"{name} te={te} {conv} vs the mesh as generated")


@pytest.mark.gpu
def test_numbering_with_tile_major_rows_and_per_point_forward_backward():
    """reorder="tile" on a mesh small enough to default to the caller's order, results back through to_caller_order; and
    model(x_eval, elem_id) on the rotated, mixed-orientation mesh with the cotangents of
    test_quad4.py::test_quad4_kernels_match_the_autograd_oracle."""
    from oracle import quad4 as Q, ref_chain as R
    name = "S:mixed"
    for conv in CONVS:
        m = _new_model(name, _dev(), reorder="tile")
        assert m.row_order == "tile" and m._perm_u is not None
        assert _slot3_populated(m.tile_plan(800).stats)
        _assert_close(_run(_lf(tile_elems=800, grad_convention=conv), m), _oracle(name, conv), f"{name} tile-major {conv}")
    name = "T:mixed"
    (nc, conn, geom, bc, mn, edges), _ = _mesh(name)
    m = _new_model(name, _dev())
    assert m.row_order == "tile"                                      # 4312 nodes: tile-major by default
    g = torch.Generator().manual_seed(5)
    M = 700
    x_eval = torch.rand(M, 2, generator=g, dtype=F64) * 2 - 1
    elem_id = torch.randint(0, conn.shape[0], (M,), generator=g)
    cu, cd, cg = (torch.randn(s, generator=g, dtype=F64) for s in ((M, 2), (M,), (M, 2, 2)))
    d = _dev()
    m.zero_grad(set_to_none=True)
    u_h, detJ, grad_u = m(x_eval.to(d), elem_id.to(d))
    ((u_h * cu.to(d)).sum() + (detJ * cd.to(d)).sum() + (grad_u * cg.to(d)).sum()).backward()
    xf = nc[~geom].clone().requires_grad_(True)
    uf = _u_caller(name, ~bc).clone().requires_grad_(True)
    X = R.assemble_coords(nc.shape[0], ~geom, xf, geom, nc[geom])
    U = R.assemble_u(nc.shape[0], ~bc, uf, bc, torch.tensor(0.0, dtype=F64))
    ru, rd, rg = Q.quad4_forward(X, U, conn, x_eval, elem_id)
    ((ru * cu).sum() + (rd * cd).sum() + (rg * cg).sum()).backward()
    assert (rd < 0).any() and (rd > 0).any()                          # both orientations were sampled
    np.testing.assert_allclose(u_h.detach().cpu().numpy(), ru.detach().numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(detJ.detach().cpu().numpy(), rd.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(grad_u.detach().cpu().numpy(), rg.detach().numpy(), rtol=1e-10, atol=1e-14)
    gx, gu = _grads(m)
    assert (gx - xf.grad).abs().max() <= 1e-10 * xf.grad.abs().max()
    assert (gu - uf.grad).abs().max() <= 1e-10 * uf.grad.abs().max()


# ---------------------------------------------------------------- d. deterministic kernel on irregular fans
@pytest.mark.gpu
def test_deterministic_kernel_on_irregular_fans():
    """The node-centric fixed-order kernel walks every node's (element, corner) list: 1 to 11 entries here.  Only the
    Dirichlet nodes have fixed coordinates, so the rows of the valence-11 node and of boundary nodes of valence 1 and 2 are
    free in both parameter tensors."""
    name = "T:mixed"
    (nc, conn, geom, bc, mn, edges), _ = _mesh(name)
    val = QM.valence(conn.numpy(), nc.shape[0])
    free = ~bc.numpy()
    assert val.max() == 11 and free[val == 11].all()
    assert (free & (val == 1)).any() and (free & (val == 2)).any()
    m = _new_model(name, _dev(), x_fixed="bc")
    assert m.node_coords_free.shape[0] == int(free.sum()) == m.u_free.shape[0]
    for conv in CONVS:
        for hasb in (False, True):
            lf = _lf(grad_convention=conv, deterministic=True)
            bf = _bf_gpu if hasb else None
            got = _run(lf, m, bf)
            _assert_close(got, _oracle(name, conv, hasb, x_fixed="bc"), f"deterministic {conv} body={hasb}")
            again = _run(lf, m, bf)
            assert again[0] == got[0] and torch.equal(again[1], got[1]) and torch.equal(again[2], got[2])


# ---------------------------------------------------------------- e./f. CG apply, block Jacobi, AMG assembly
def _sample_nodes(name, plan, count=32):
    """`count` nodes with free u rows (ids of mesh `name`): the highest- and lowest-valence ones, nodes on a tile border
    (touched by home elements of more than one tile, from plan.tile_elements) and a random rest."""
    (nc, conn, geom, bc, mn, edges), _ = _mesh(name)
    cn = conn.numpy()
    free = ~bc.numpy()
    val = QM.valence(cn, nc.shape[0])
    ids = np.nonzero(free)[0]
    order = ids[np.argsort(val[ids], kind="stable")]
    picked = [int(order[-1]), int(order[-2]), int(order[0]), int(order[1])]
    tiles_at = np.zeros(nc.shape[0], dtype=np.int64)
    for t in range(plan.n_tiles):
        gid, _, home = plan.tile_elements(t)
        tiles_at[np.unique(cn[gid[home]])] += 1
    assert sorted(plan.export("owned_node_ids").tolist()) == list(range(nc.shape[0]))      # every node owned exactly once
    border = np.nonzero((tiles_at >= 2) & free)[0]
    assert plan.n_tiles == 1 or len(border) >= 12
    picked += [int(b) for b in border[np.linspace(0, len(border) - 1, 12).astype(int)] if int(b) not in picked]
    rest = [int(i) for i in np.random.default_rng(7).permutation(ids) if int(i) not in picked]
    picked = np.array(picked + rest[: count - len(picked)])
    assert len(picked) == count == len(set(picked.tolist())) and (tiles_at[picked] >= 2).sum() >= 8
    assert val[picked].max() == val[ids].max() and val[picked].min() == val[ids].min()
    return picked


def _oracle_columns(name, nodes, conv):
    """K e_(i, c) for the sampled nodes i and c = x, y as the oracle's dE/du at u = e_(i, c) (E is quadratic in u: no forces,
    u_fixed = 0), on the cells that touch a sampled node -- the energy is a sum over cells and no other cell sees node i.
    -> [len(nodes), 2, Nn, 2] by node id."""
    from oracle import quad4 as Q, ref_chain as R
    (nc, conn, geom, bc, mn, edges), _ = _mesh(name)
    sub = conn[torch.from_numpy(np.isin(conn.numpy(), nodes).any(axis=1))]
    out = torch.zeros(len(nodes), 2, nc.shape[0], 2, dtype=F64)
    for k, i in enumerate(nodes):
        for c in range(2):
            U = torch.zeros(nc.shape[0], 2, dtype=F64)
            U[i, c] = 1.0
            U.requires_grad_(True)
            (out[k, c],) = torch.autograd.grad(Q.quad4_domain_energy(nc, U, sub, R.plane_stress_C(), None, conv), U)
    return out


def _oracle_Kp(name, conv, p_caller):
    """K p over the free u rows (caller order) = the oracle's dE/du at u = p with no forces and u_fixed = 0."""
    return _oracle(name, conv, with_edges=False, u=p_caller)[2]


@pytest.mark.gpu
@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("name,te", [("S", 600), ("S", 800), ("T:mixed", 0), ("T:mixed", 800)], ids=["S600", "S800", "T0", "T800"])
def test_cg_apply_and_block_jacobi_per_branch(name, te, conv):
    from hidenn_fem_amd.solve import Quad4FrozenMeshSolver
    from test_gpu_solve_quad4 import _check_apply
    mesh, _ = _mesh(name)
    bc = mesh[3]
    m = _new_model(name, _dev(), conv=conv)
    lf = _lf(tile_elems=te)
    plan = m.tile_plan(te)
    assert quad4_cg_apply_branch(plan.stats) == ("<4,4>" if te == 800 else "<3,3>"), plan.stats
    assert _slot3_populated(plan.stats) == (te == 800)
    _check_apply(m, lf)                                              # against the energy kernel on the same plan, 1e-12
    s = Quad4FrozenMeshSolver(m, lf)
    p = torch.randn(int((~bc).sum()), 2, dtype=F64, generator=torch.Generator().manual_seed(3)) * 1e-4
    q, _ = s.apply(m.from_caller_order(p.to(_dev()), "u").contiguous())
    q = m.to_caller_order(q, "u").cpu()
    want = _oracle_Kp(name, conv, p)
    err = (q - want).abs().max().item() / want.abs().max().item()
    print(f"apply vs oracle K p ({name}, {te}, {conv}): {err:.3e}")
    assert err <= 1e-10
    # block Jacobi: the 2 x 2 diagonal blocks against oracle columns, at the tolerance of
    # test_gpu_solve_quad4.py::test_block_jacobi_blocks_match_the_oracle_hessian
    nodes = _sample_nodes(name, plan)
    cols = _oracle_columns(name, nodes, conv)
    idx = torch.arange(len(nodes))
    blk = cols[idx, :, torch.from_numpy(nodes), :]                   # [k, c (column), r (row)]
    want = torch.stack([blk[:, 0, 0], 0.5 * (blk[:, 0, 1] + blk[:, 1, 0]), blk[:, 1, 1]], dim=1)
    s.refresh()
    row_of = torch.cumsum(~bc, 0) - 1                                # caller row of a node id
    got = m.to_caller_order(s.diag, "u").cpu()[row_of[torch.from_numpy(nodes)]]
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"block Jacobi ({name}, {te}, {conv}): {err:.3e}")
    assert err <= 1e-12


def _bsr_matvec(crow, col, vals, p):
    """K p from the BSR arrays in numpy: p, result [n, 2]."""
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    out = np.zeros_like(p)
    np.add.at(out, rows, np.einsum("kab,kb->ka", vals, p[col]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("conv", CONVS)
def test_amg_fine_level_assembly_on_irregular_fans(conv):
    """assemble_stiffness (one thread per block row walking the row's fan: 1 to 11 cells here) on the renumbered
    mixed-orientation split mesh: symmetric, the sampled oracle columns, K_ff p for three random p, two assemblies the same
    bits.  Tolerances of test_gpu_solve_quad4.py::test_assembled_stiffness_equals_the_oracle_hessian_...  Symmetry is not
    bitwise: block (a, b) comes from the element gradient at a unit displacement of a, block (b, a) from one at b, two
    different roundings of the same sum of at most 11 cells x 4 Gauss points (measured 1.3e-16 max|K|).  The bound is
    1e-13 max|K|, ten times below the 1e-12 the matrix is held to against the oracle: 44 terms at ~10 eps max|K| each."""
    from hidenn_fem_amd.solve import assemble_stiffness
    name = "T:mixed"
    mesh, _ = _mesh(name)
    bc = mesh[3]
    m = _new_model(name, _dev(), conv=conv)
    lf = _lf()
    K = assemble_stiffness(m, lf)
    assert K.layout == torch.sparse_bsr and K.dtype == F64 and K.values().shape[1:] == (2, 2)
    K2 = assemble_stiffness(m, lf)
    assert torch.equal(K.values(), K2.values()) and torch.equal(K.col_indices(), K2.col_indices())
    crow, col, vals = K.crow_indices().cpu().numpy(), K.col_indices().cpu().numpy(), K.values().cpu().numpy()
    n = len(crow) - 1
    assert n == int((~bc).sum())
    rows = np.repeat(np.arange(n), np.diff(crow))
    assert np.diff(crow).min() < 9 < np.diff(crow).max()              # not the 9-point pattern of a structured grid
    # symmetry: block (r, c) is the transpose of block (c, r), and the pattern holds both
    pos = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(rows, col))}
    mate = np.array([pos[(int(c), int(r))] for r, c in zip(rows, col)])
    asym = np.abs(vals - vals[mate].transpose(0, 2, 1)).max() / np.abs(vals).max()
    print(f"assembled K_ff ({conv}): {n} block rows, {len(col)} blocks, max asymmetry / max|K| = {asym:.3e}")
    assert asym <= 1e-13
    to_storage = lambda a: m.from_caller_order(a, "u").numpy()       # CPU tensors in, numpy out
    to_caller = lambda a: m.to_caller_order(torch.from_numpy(a), "u")
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        p = torch.randn(n, 2, dtype=F64, generator=g)
        got = to_caller(_bsr_matvec(crow, col, vals, to_storage(p)))
        want = _oracle_Kp(name, conv, p)
        err = (got - want).abs().max().item() / want.abs().max().item()
        print(f"K_ff p vs oracle ({conv}): {err:.3e}")
        assert err <= 1e-12
    nodes = _sample_nodes(name, m.tile_plan(0))
    cols = _oracle_columns(name, nodes, conv)[:, :, ~bc, :]          # [k, c, free rows (caller order), 2]
    row_of = torch.cumsum(~bc, 0) - 1
    scale = cols.abs().max().item()
    worst = 0.0
    for k, i in enumerate(nodes):
        for c in range(2):
            e = torch.zeros(n, 2, dtype=F64)
            e[row_of[i], c] = 1.0
            got = to_caller(_bsr_matvec(crow, col, vals, to_storage(e)))
            worst = max(worst, (got - cols[k, c]).abs().max().item())
    print(f"assembled columns vs oracle ({conv}): {worst / scale:.3e}")
    assert worst <= 1e-12 * scale


# ---------------------------------------------------------------- g. mesh kernels on the same inputs
@pytest.mark.gpu
@pytest.mark.parametrize("orient", ["cw", "mixed"])
def test_mesh_kernels_on_renumbered_split_mesh(orient):
    from hidenn_fem_amd.radapt import quad4_max_feasible_step, quad4_quality_barrier
    from test_gpu_radapt import _caller_rows
    from test_gpu_radapt_quad4 import _barrier_torch, _check_measure, _perturb
    from test_radapt_quad4_host import quad4_corners_np, quad4_step_bound_np
    m = _new_model(f"T:{orient}", _dev())
    mq, q = _check_measure(m)
    assert mq.n_inverted == 0 and mq.min_q > 0.0 and mq.min_det_ratio == 1.0 and (q > 0).all()
    _perturb(m, 0.05, seed=9)
    mq, _ = _check_measure(m)
    assert mq.n_inverted == 0
    conn = m.connectivity.cpu().numpy()
    g = torch.Generator().manual_seed(5)
    for eta in (0.25, 0.6):
        d = torch.randn(m.node_coords_free.shape, generator=g, dtype=F64).to(_dev())
        got = quad4_max_feasible_step(m, d, eta=eta)
        X, D = _caller_rows(m), _caller_rows(m, d)
        want = quad4_step_bound_np(X[conn], D[conn], eta)[0].min()
        assert math.isfinite(got) and abs(got - want) <= 1e-12 * want, (eta, got, want)
        c0, _ = quad4_corners_np(X[conn])
        c1, _ = quad4_corners_np((X + got * D)[conn])
        assert abs((c1 / c0).min() - eta) <= 1e-10, (eta, (c1 / c0).min())
    w = 0.7
    val, gq = quad4_quality_barrier(m, w)
    want_v, want_g = _barrier_torch(m.coords.detach().double().cpu(), m.initial_node_coords.double().cpu(),
                                    m.connectivity.cpu(), m._idx_free.long().cpu(), w)
    assert want_v > 0.0
    assert abs(val.item() - want_v) <= 1e-11 * abs(want_v)
    assert (gq.cpu() - want_g).abs().max().item() <= 1e-11 * want_g.abs().max().item()
