"""The 14 kernel instances of csrc/recover.hip -- stress_recover_kernel<3|4, Law> and zz_error_kernel<3|4, Law> for
LinearLaw<false>, LinearLaw<true> and CauchyLaw, zz_finish_kernel<false|true> -- at their size, valence and inversion edges,
through the raw C ABI on the hand-built cases of tests/recovery_cases.py (pinned on the CPU by tests/test_recovery_cases_host.py)
against the CPU statements tests/zz_reference.py and tests/hyper_zz_reference.py.

Every output is pre-filled with NaN and carries a guard tail of 64 sentinel doubles; ``partials`` has exactly one double2
(linear) or two (finite strain) per block before its guard.

Tolerances are the project's parity tolerances of tests/test_gpu_stress_recovery.py and tests/test_gpu_hyper_stress_recovery.py,
for their reason (the kernels and the statements differ in summation order and fma contraction only): nodal stress, nodal J and
lumped area 1e-11 of the maximum; eta_e^2 and the per-element norm2 1e-10 of the maximum over the finite entries; the two totals,
eta and relative 1e-11 relative; min det F 1e-13 absolute; the inverted count exact.  Where sigma* = sigma_h (``RC.is_patch``) eta
is judged by relative <= 1e-12, as the patch tests of those files do, and not by a ratio against a rounding-size eta2.  The totals
against ``math.fsum`` of the device's own per-element arrays: 1e-12 relative -- the terms are non-negative and the device's tree
(wave shuffles, four waves, at most two trips, the finish tree) has about 20 levels, each within eps = 1.1e-16 relative."""
import ctypes as C
import math

import pytest
import torch

import recovery_cases as RC
from oracle import ref_chain as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = torch.device("cuda:0")
SENTINEL = -7.03125
PHYSICAL = 64                                   # HFEM_FLAG_PHYSICAL_GRAD
CASES = [(kind, law, name) for kind in RC.KINDS for law in RC.LAWS for name in RC.names(kind, law)]

_cache = {}


def lib():
    from hidenn_fem_amd import _lib
    return _lib.lib()


def stream():
    from hidenn_fem_amd import _lib
    return _lib.stream_ptr(DEV)


def material(law):
    if law == "cauchy":
        return (C.c_double * 2)(RC.LAM, RC.MU)
    Cm = R.plane_stress_C()
    return (C.c_double * 4)(Cm[0, 0].item(), Cm[0, 1].item(), Cm[1, 1].item(), Cm[2, 2].item())


class Guarded:
    """n doubles of NaN and, past them, RC.GUARD doubles of the sentinel."""

    def __init__(self, n, fill=float("nan")):
        self.n = n
        self.full = torch.full((n + RC.GUARD,), SENTINEL, dtype=F64, device=DEV)
        self.full[:n] = fill
        self.ptr = self.full.data_ptr()

    def read(self, what):
        got = self.full.cpu()
        tail = got[self.n:]
        assert torch.equal(tail.view(torch.int64), torch.full_like(tail, SENTINEL).view(torch.int64)), f"{what}: guard overwritten"
        return got[:self.n]


def inputs(kind, name, finite):
    """The case on the device: uploaded once per case, never modified."""
    key = ("in", kind, name, finite)
    if key not in _cache:
        c = RC.case(kind, name, finite)
        adj_ptr, adj = RC.adjacency(c)
        _cache[key] = tuple(x.contiguous().to(DEV) for x in (c.coords, c.u, c.conn.to(torch.int32), adj_ptr, adj))
    return _cache[key]


def run(kind, law, name, area=True, nodal_J=True, norm2=True):
    """Recover, then the ZZ kernels on the recovered stress, as the classes of hidenn_fem_amd.post call them.  -> dict of CPU
    tensors (absent outputs: None).  Asserts here: both calls return 0, every guard is bitwise intact."""
    L, st = lib(), stream()
    finite = law == "cauchy"
    c = RC.case(kind, name, finite)
    nn, ne = c.coords.shape[0], c.conn.shape[0]
    nb = RC.blocks(ne)
    X, U, conn32, adj_ptr, adj = inputs(kind, name, finite)
    mat = material(law)
    o = dict(sig=Guarded(3 * nn), area=Guarded(nn) if area else None, J=Guarded(nn) if finite and nodal_J else None,
             eta2=Guarded(ne), norm2=Guarded(ne) if norm2 else None, partials=Guarded((4 if finite else 2) * nb),
             totals=Guarded(4 if finite else 2))
    p = {k: (v.ptr if v is not None else None) for k, v in o.items()}
    if finite:
        rc = getattr(L, f"hfem_{kind}_hyper_stress_recover")(0, X.data_ptr(), U.data_ptr(), conn32.data_ptr(), ne, nn, adj_ptr.data_ptr(),
                                                             adj.data_ptr(), mat, p["sig"], p["J"], p["area"], st)
        assert rc == 0, L.hfem_last_error()
        rc = getattr(L, f"hfem_{kind}_hyper_zz_error")(0, X.data_ptr(), U.data_ptr(), conn32.data_ptr(), ne, p["sig"], mat, p["eta2"],
                                                       p["norm2"], p["partials"], p["totals"], st)
    else:
        flags = PHYSICAL if law == "physical" else 0
        rc = getattr(L, f"hfem_{kind}_stress_recover")(0, X.data_ptr(), U.data_ptr(), conn32.data_ptr(), ne, nn, adj_ptr.data_ptr(),
                                                       adj.data_ptr(), mat, flags, p["sig"], p["area"], st)
        assert rc == 0, L.hfem_last_error()
        rc = getattr(L, f"hfem_{kind}_zz_error")(0, X.data_ptr(), U.data_ptr(), conn32.data_ptr(), ne, p["sig"], mat, flags, p["eta2"],
                                                 p["norm2"], p["partials"], p["totals"], st)
    assert rc == 0, L.hfem_last_error()
    torch.cuda.synchronize()
    out = {k: (v.read(f"{kind} {law} {name} {k}") if v is not None else None) for k, v in o.items()}
    out["sig"] = out["sig"].reshape(nn, 3)
    return out


def device(kind, law, name):
    """The device result of one (case, law) with every output asked for: computed once, shared, never modified."""
    key = ("out", kind, law, name)
    if key not in _cache:
        _cache[key] = run(kind, law, name)
    return _cache[key]


def live_nodes(c):
    """bool [nn]: the nodes that some element which is not inverted lists."""
    keep = torch.ones(c.conn.shape[0], dtype=torch.bool)
    keep[c.meta["inverted"]] = False
    mask = torch.zeros(c.coords.shape[0], dtype=torch.bool)
    mask[c.conn[keep].reshape(-1)] = True
    return mask


def rel_max(got, ref):
    """max |got - ref| / max |ref|; a reference that is zero throughout wants exact zeros (0.0 then, else inf)."""
    top = ref.abs().max().item() if ref.numel() else 0.0
    if top == 0.0:
        return 0.0 if (got == 0.0).all() else float("inf")
    return (got - ref).abs().max().item() / top


def rel(a, b):
    if b == 0.0:
        return 0.0 if a == 0.0 else float("inf")
    return abs(a - b) / abs(b)


def summary(tot, finite):
    """eta, relative as hidenn_fem_amd.post forms them from the totals."""
    e2, n2 = tot[0].item(), tot[1].item()
    count = int(tot[3].item()) if finite else 0
    relative = 1.0 if count > 0 else ((e2 / (n2 + e2)) ** 0.5 if n2 + e2 > 0.0 else 0.0)
    return e2 ** 0.5, relative


@pytest.mark.parametrize("kind,law,name", CASES)
def test_parity_with_the_cpu_statement(kind, law, name):
    finite = law == "cauchy"
    c, ref, got = RC.case(kind, name, finite), RC.reference(kind, name, law), device(kind, law, name)
    nn, ne = c.coords.shape[0], c.conn.shape[0]
    # every live entry was written: no NaN is left anywhere (an inverted element's eta2 is +inf, never NaN)
    for k, v in got.items():
        if v is not None:
            assert not torch.isnan(v).any(), f"{k}: NaN left"
    for k in ("sig", "area", "norm2") + (("J",) if finite else ()):
        assert torch.isfinite(got[k]).all(), k
    # a node of no element, or of inverted elements only: exactly zero, area 0, J 0
    dead = ~live_nodes(c)
    assert (got["sig"][dead] == 0.0).all() and (got["area"][dead] == 0.0).all() and (got["area"][~dead] > 0.0).all()
    if finite:
        assert (got["J"][dead] == 0.0).all()
    fin = torch.isfinite(ref["eta2"])
    assert torch.equal(torch.isfinite(got["eta2"]), fin) and (got["eta2"][~fin] == float("inf")).all()
    eta, relative = summary(got["totals"], finite)
    fig = dict(sigma=rel_max(got["sig"], ref["nodal_stress"]), area=rel_max(got["area"], ref["area"]),
               norm2=rel_max(got["norm2"], ref["norm2"]), norm2_total=rel(got["totals"][1].item(), ref["norm2_total"]))
    if finite:
        fig.update(J=rel_max(got["J"], ref["nodal_J"]), min_J=abs(got["totals"][2].item() - ref["min_J"]))
    patch = RC.is_patch(kind, name)
    if patch:
        e2 = math.fsum(got["eta2"][fin].tolist())
        fig["patch_relative"] = (e2 / (got["totals"][1].item() + e2)) ** 0.5
    else:
        fig["eta2"] = rel_max(got["eta2"][fin], ref["eta2"][fin])
        if not c.meta["inverted"]:
            fig.update(eta=rel(eta, ref["eta"]), relative=rel(relative, ref["relative"]))
    print(kind, law, name, f"nn {nn} ne {ne}", {k: f"{v:.2e}" for k, v in fig.items()}, f"eta_rel {relative:.4f}")
    assert fig["sigma"] <= 1e-11 and fig["area"] <= 1e-11 and fig.get("J", 0.0) <= 1e-11
    assert fig["norm2"] <= 1e-10 and fig.get("eta2", 0.0) <= 1e-10
    assert fig["norm2_total"] <= 1e-11 and fig.get("eta", 0.0) <= 1e-11 and fig.get("relative", 0.0) <= 1e-11
    assert fig.get("patch_relative", 0.0) <= 1e-12
    assert fig.get("min_J", 0.0) <= 1e-13
    if finite:
        assert got["totals"][3].item() == float(ref["inverted"]) == float(len(c.meta["inverted"]))
    if c.meta["inverted"]:
        assert got["totals"][0].item() == float("inf") and math.isinf(eta) and relative == 1.0 == ref["relative"]
    elif patch:
        assert got["totals"][1].item() > 0.0 and relative <= 1e-12


@pytest.mark.parametrize("kind,law,name", CASES)
def test_totals_are_the_sums_of_their_own_arrays(kind, law, name):
    """At ne = 65 537 this fails if the finish kernel drops its 257th partial: the last element's share is above 1e-8 of the
    eta2 total and above 1e-5 of the norm2 total (tests/test_recovery_cases_host.py)."""
    finite = law == "cauchy"
    c, got = RC.case(kind, name, finite), device(kind, law, name)
    e2, n2 = got["totals"][0].item(), got["totals"][1].item()
    fin = torch.isfinite(got["eta2"])
    own_e, own_n = math.fsum(got["eta2"][fin].tolist()), math.fsum(got["norm2"].tolist())
    print(kind, law, name, f"eta2 {e2:.15e} own {own_e:.15e}  norm2 {n2:.15e} own {own_n:.15e} rel {rel(n2, own_n):.2e}")
    assert rel(n2, own_n) <= 1e-12
    if c.meta["inverted"]:
        assert e2 == float("inf") and int((~fin).sum()) == len(c.meta["inverted"])
    else:
        assert rel(e2, own_e) <= 1e-12
    # the partials, which the finish kernel reads: block b's are the sums over its own 256 elements
    nb = RC.blocks(c.conn.shape[0])
    part = got["partials"].reshape(nb, 4 if finite else 2)
    for b in sorted({0, nb // 2, nb - 1}):
        rows = slice(b * RC.BLOCK, min((b + 1) * RC.BLOCK, c.conn.shape[0]))
        assert rel(part[b, 1].item(), math.fsum(got["norm2"][rows].tolist())) <= 1e-12
        if fin[rows].all():
            assert rel(part[b, 0].item(), math.fsum(got["eta2"][rows].tolist())) <= 1e-12
        if finite:
            assert part[b, 3].item() == float((~fin[rows]).sum())


@pytest.mark.parametrize("kind", RC.KINDS)
def test_finite_strain_minimum_and_count_through_the_second_trip(kind):
    """ne = 65 537, 257 partials: what the finish kernel's thread 0 carries from its first trip into its second."""
    J = {name: RC.reference(kind, name, "cauchy")["J"] for name in RC.TWIN_NAMES}
    last = 4 * 256                                                   # block 256's {eta2, norm2, min det F, count}
    # the minimum of all is element 65 536's: it arrives in the second trip
    ref, got = RC.reference(kind, "twin_min_last", "cauchy"), device(kind, "cauchy", "twin_min_last")
    assert ref["min_J"] == J["twin_min_last"][RC.LAST].min().item() and ref["inverted"] == 0
    assert abs(got["totals"][2].item() - ref["min_J"]) <= 1e-13 and got["totals"][3].item() == 0.0
    # variant 1: the valid minimum in the last block; inverted elements in blocks 0, 128 and 255: the count is 3, the minimum theirs
    ref, got = RC.reference(kind, "twin_inverted_elsewhere", "cauchy"), device(kind, "cauchy", "twin_inverted_elsewhere")
    assert got["totals"][3].item() == 3.0 and abs(got["totals"][2].item() - ref["min_J"]) <= 1e-13 and ref["min_J"] < 0.0
    assert abs(got["partials"][last + 2].item() - J["twin_inverted_elsewhere"][RC.LAST].min().item()) <= 1e-13
    assert got["partials"][last + 3].item() == 0.0 and math.isfinite(got["eta2"][RC.LAST].item())
    assert torch.isinf(got["eta2"]).nonzero().flatten().tolist() == RC.case(kind, "twin_inverted_elsewhere", True).meta["inverted"]
    # variant 2: element 65 536 is one of the three
    ref, got = RC.reference(kind, "twin_inverted_last", "cauchy"), device(kind, "cauchy", "twin_inverted_last")
    assert got["totals"][3].item() == 3.0 and got["eta2"][RC.LAST].item() == float("inf") and got["norm2"][RC.LAST].item() == 0.0
    assert got["partials"][last + 3].item() == 1.0 and got["partials"][last].item() == float("inf")
    assert abs(got["partials"][last + 2].item() - J["twin_inverted_last"][RC.LAST].min().item()) <= 1e-13
    assert abs(got["totals"][2].item() - ref["min_J"]) <= 1e-13
    assert torch.isinf(got["eta2"]).nonzero().flatten().tolist() == RC.case(kind, "twin_inverted_last", True).meta["inverted"]


@pytest.mark.parametrize("kind", RC.KINDS)
def test_det_F_of_exactly_zero_is_inverted(kind):
    """j == -1.0 is the boundary of the rule j > -1: inverted.  Nothing is NaN; the one element's nodes have nothing to recover."""
    got = device(kind, "cauchy", "det_zero")
    assert got["totals"].tolist() == [float("inf"), 0.0, 0.0, 1.0]
    assert got["eta2"].tolist() == [float("inf")] and got["norm2"].tolist() == [0.0]
    assert (got["sig"] == 0.0).all() and (got["area"] == 0.0).all() and (got["J"] == 0.0).all()
    assert got["partials"].tolist() == [float("inf"), 0.0, 0.0, 1.0]


def test_one_inverted_point_inverts_the_cell():
    got, ref = device("quad4", "cauchy", "one_point"), RC.reference("quad4", "one_point", "cauchy")
    assert torch.isinf(got["eta2"]).tolist() == [False] * 4 + [True] + [False] * 4 and got["totals"][3].item() == 1.0
    assert abs(got["totals"][2].item() - ref["J"][4].min().item()) <= 1e-13 and got["norm2"][4].item() == 0.0
    assert (got["area"] > 0.0).all()                                  # the cell's nodes keep their valid neighbours' values


@pytest.mark.parametrize("kind", RC.KINDS)
def test_a_node_of_inverted_elements_only(kind):
    c, ref, got = RC.case(kind, "end_inverted", True), RC.reference(kind, "end_inverted", "cauchy"), device(kind, "cauchy", "end_inverted")
    dead, shared = c.meta["dead"], c.meta["shared"]
    assert (got["sig"][dead] == 0.0).all() and (got["area"][dead] == 0.0).all() and (got["J"][dead] == 0.0).all()
    one = ref["sig_h"][0, 0]                                          # the valid element's one stress: the shared nodes get it alone
    assert (got["sig"][shared] - one).abs().max().item() <= 1e-11 * one.abs().max().item()
    assert (got["J"][shared] - 1.25 * 1.125).abs().max().item() <= 1e-11 * 1.25 * 1.125
    assert rel_max(got["area"][shared], ref["area"][shared]) <= 1e-11


@pytest.mark.parametrize("law", RC.LAWS)
@pytest.mark.parametrize("kind", RC.KINDS)
def test_null_outputs_change_nothing_else(kind, law):
    """nodal_area and nodal_J null or not (the linear entry points have no nodal_J), norm2 null or not, at nn = 257."""
    full = device(kind, law, "nn257")
    combos = [(a, j) for a in (False, True) for j in ((False, True) if law == "cauchy" else (True,))]
    assert len(combos) == (4 if law == "cauchy" else 2)
    for a, j in combos:
        got = run(kind, law, "nn257", area=a, nodal_J=j, norm2=a)
        assert torch.equal(got["sig"], full["sig"]) and torch.equal(got["eta2"], full["eta2"]) and torch.equal(got["totals"], full["totals"])
        assert (got["area"] is None) == (not a) and (a is False or torch.equal(got["area"], full["area"]))
        assert (got["norm2"] is None) == (not a) and (a is False or torch.equal(got["norm2"], full["norm2"]))
        if law == "cauchy":
            assert (got["J"] is None) == (not j) and (j is False or torch.equal(got["J"], full["J"]))


@pytest.mark.parametrize("name", ["ne65537", "fan_big"])
@pytest.mark.parametrize("law", RC.LAWS)
@pytest.mark.parametrize("kind", RC.KINDS)
def test_two_calls_are_bitwise_equal(kind, law, name):
    a, b = device(kind, law, name), run(kind, law, name)
    for k, v in a.items():
        assert (v is None and b[k] is None) or torch.equal(v.view(torch.int64), b[k].view(torch.int64)), k


def test_refusals_and_empty_calls():
    """A negative count is refused whatever the other count is, on all eight entry points; a zero count returns 0 and touches
    nothing."""
    L, st = lib(), stream()
    z = torch.zeros(64, dtype=F64, device=DEV)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, pi = z.data_ptr(), zi.data_ptr()
    outs = [Guarded(64, fill=SENTINEL) for _ in range(4)]
    a, b, c, d = (o.ptr for o in outs)
    for kind in RC.KINDS:
        lin_rec, lin_zz = getattr(L, f"hfem_{kind}_stress_recover"), getattr(L, f"hfem_{kind}_zz_error")
        hyp_rec, hyp_zz = getattr(L, f"hfem_{kind}_hyper_stress_recover"), getattr(L, f"hfem_{kind}_hyper_zz_error")
        mat, lame = material("physical"), material("cauchy")
        for ne, nn in ((-1, 0), (0, -1), (-1, 5), (5, -1), (-1, -1)):
            assert lin_rec(0, p, p, pi, ne, nn, pi, pi, mat, 0, a, b, st) < 0 and b"negative" in L.hfem_last_error(), (kind, ne, nn)
            assert hyp_rec(0, p, p, pi, ne, nn, pi, pi, lame, a, b, c, st) < 0 and b"negative" in L.hfem_last_error(), (kind, ne, nn)
        assert lin_zz(0, p, p, pi, -1, p, mat, 0, a, b, c, d, st) < 0 and b"negative" in L.hfem_last_error()
        assert hyp_zz(0, p, p, pi, -1, p, lame, a, b, c, d, st) < 0 and b"negative" in L.hfem_last_error()
        for ne, nn in ((0, 5), (5, 0), (0, 0)):
            assert lin_rec(0, p, p, pi, ne, nn, pi, pi, mat, 0, a, b, st) == 0
            assert hyp_rec(0, p, p, pi, ne, nn, pi, pi, lame, a, b, c, st) == 0
        assert lin_zz(0, p, p, pi, 0, p, mat, 0, a, b, c, d, st) == 0
        assert hyp_zz(0, p, p, pi, 0, p, lame, a, b, c, d, st) == 0
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert (o.read(f"output {i}") == SENTINEL).all(), "a refused or empty call wrote an output"
