"""The case builders of tests/recovery_cases.py, checked on the CPU: what tests/test_gpu_recovery_edges.py relies on -- the counts
and the block counts they imply, which nodes are referenced, the valences and the hub's corners, where the minimum det F and the
inverted elements sit, the exact det F == 0, the one-point pattern, and that no other det F comes within 0.05 of zero -- so that
a broken builder fails here and not on the card.  Both CPU statements run on every case."""
import math

import numpy as np
import pytest
import torch

import recovery_cases as RC

F64 = torch.float64
ALL = [(kind, law, name) for kind in RC.KINDS for law in RC.LAWS for name in RC.names(kind, law)]
FINITE = [(kind, name) for kind in RC.KINDS for name in RC.finite_names(kind)]


def valence(c):
    adj_ptr, _ = RC.adjacency(c)
    return (adj_ptr[1:] - adj_ptr[:-1]).long()


def test_the_sizes_are_the_ones_the_kernels_change_form_at():
    assert RC.BLOCK == 256 and RC.NE_COUNTS == (1, 255, 256, 257, 65536, 65537) and RC.NN_COUNTS == (255, 256, 257)
    assert [RC.blocks(n) for n in RC.NE_COUNTS] == [1, 1, 1, 2, 256, 257]          # 256: one partial per finish thread; 257: a 2nd trip
    assert [RC.blocks(n) for n in RC.NN_COUNTS] == [1, 1, 2]
    assert RC.LAST == 65536 and RC.LAST // RC.BLOCK == 256 and RC.blocks(RC.NE_BIG) - 1 == 256
    for kind in RC.KINDS:
        coords, conn = RC.count_mesh(kind)
        assert conn.shape == (65792, RC.NPE[kind]) and coords.dtype == F64
        for n in RC.NE_COUNTS:
            c = RC.case(kind, f"ne{n}", False)
            assert c.conn.shape == (n, RC.NPE[kind]) and torch.equal(c.conn, conn[:n]) and c.coords.shape == coords.shape
            assert not RC.referenced(c).all()                                     # unreferenced nodes stay in coords
        assert torch.equal(RC.case(kind, "patch65537", False).conn, conn[:65537])
        assert torch.equal(RC.case(kind, "patch257", False).conn, conn[:257])
        for name in RC.TWIN_NAMES:
            assert torch.equal(RC.case(kind, name, True).conn, conn[:65537])


@pytest.mark.parametrize("kind", RC.KINDS)
def test_strips_reference_every_node(kind):
    for nn in RC.NN_COUNTS:
        c = RC.case(kind, f"nn{nn}", True)
        assert c.coords.shape == (nn, 2) and RC.referenced(c).all()
        assert c.conn.shape[0] == (nn - 2 if kind == "tri3" else {255: 126, 256: 127, 257: 127}[nn])
        v = valence(c)
        assert v.min().item() >= 1 and v.sum().item() == c.conn.numel()
    c = RC.case(kind, "nn257_orphan", True)
    ref = RC.referenced(c)
    assert c.coords.shape == (257, 2) and ref[:256].all() and not ref[256] and valence(c)[256].item() == 0
    if kind == "quad4":
        # the odd counts' extra cell shares exactly one node with the strip, and every local corner starts a listing
        for nn in (255, 257):
            c = RC.case(kind, f"nn{nn}", True)
            last = set(c.conn[-1].tolist())
            assert len(last & set(c.conn[:-1].reshape(-1).tolist())) == 1
        c = RC.case(kind, "nn256", True)
        assert torch.equal(c.conn[0], torch.tensor([0, 2, 3, 1])) and torch.equal(c.conn[1], torch.tensor([4, 5, 3, 2]))


@pytest.mark.parametrize("kind", RC.KINDS)
def test_fans_hub_valence_and_corners(kind):
    npe = RC.NPE[kind]
    for name, n in (("fan3", 3), ("fan_big", RC.FAN_BIG[kind])):
        c = RC.case(kind, name, True)
        hub = c.meta["hub"]
        adj_ptr, adj = RC.adjacency(c)
        v = valence(c)
        assert c.conn.shape == (n, npe) and RC.referenced(c).all()
        assert v[hub].item() == n and (v[1:] <= 2).all()
        mine = adj[adj_ptr[hub]:adj_ptr[hub + 1]]
        assert torch.equal(mine >> 2, torch.arange(n, dtype=torch.int32))           # ascending element id
        assert torch.equal((mine & 3).long(), torch.arange(n) % npe)                # element i lists the hub at corner i mod npe
        if n >= npe:
            assert set((mine & 3).tolist()) == set(range(npe))
        # no two elements are congruent: their sorted edge lengths differ
        X = c.coords[c.conn]
        L = torch.stack([(X[:, k] - X[:, (k + 1) % npe]).norm(dim=1) for k in range(npe)], dim=1).sort(dim=1).values
        assert (torch.cdist(L, L) + torch.eye(n, dtype=F64)).min().item() > 1e-6
    assert RC.FAN_BIG == {"tri3": 300, "quad4": 64}
    # the valence-1 end: every node of the single kept element
    c = RC.case(kind, "ne1", True)
    assert valence(c)[c.conn[0]].tolist() == [1] * npe and valence(c).sum().item() == npe


@pytest.mark.parametrize("kind,law,name", ALL)
def test_both_statements_run_on_every_case(kind, law, name):
    c = RC.case(kind, name, law == "cauchy")
    r = RC.reference(kind, name, law)
    nn, ne = c.coords.shape[0], c.conn.shape[0]
    assert r["nodal_stress"].shape == (nn, 3) and r["area"].shape == (nn,) and r["eta2"].shape == (ne,) and r["norm2"].shape == (ne,)
    bad = torch.zeros(ne, dtype=torch.bool)
    bad[c.meta["inverted"]] = True
    for key in ("nodal_stress", "area", "norm2") + (("nodal_J",) if law == "cauchy" else ()):
        assert torch.isfinite(r[key]).all(), key
    assert torch.isfinite(r["eta2"][~bad]).all() and (r["eta2"][~bad] >= 0.0).all() and (r["norm2"] >= 0.0).all()
    assert math.isfinite(r["norm2_total"])
    # a node that nothing (valid) references: zeros and area 0
    live = torch.zeros(nn, dtype=torch.bool)
    live[c.conn[~bad].reshape(-1)] = True
    assert (r["area"][live] > 0.0).all() and (r["area"][~live] == 0.0).all() and (r["nodal_stress"][~live] == 0.0).all()
    if law == "cauchy":
        assert r["inverted_mask"].nonzero().flatten().tolist() == c.meta["inverted"] and r["inverted"] == len(c.meta["inverted"])
        assert torch.isinf(r["eta2"][bad]).all() and (r["norm2"][bad] == 0.0).all() and (r["nodal_J"][~live] == 0.0).all()
        if r["inverted"]:
            assert r["relative"] == 1.0 and math.isinf(r["eta"])
    if not c.meta["inverted"]:
        if RC.is_patch(kind, name):
            assert r["relative"] <= 1e-12 and r["norm2_total"] > 0.0
        else:
            assert 1e-4 < r["relative"] < 1.0                                     # an eta well above rounding


@pytest.mark.parametrize("kind,name", FINITE)
def test_no_det_F_near_zero_outside_the_boundary_case(kind, name):
    J = RC.reference(kind, name, "cauchy")["J"]
    assert torch.isfinite(J).all()
    if name == "det_zero":
        assert (J == 0.0).all()                                                   # exactly: the boundary of j > -1
        r = RC.reference(kind, name, "cauchy")
        assert r["min_J"] == 0.0 and r["inverted"] == 1 and (r["nodal_stress"] == 0.0).all() and (r["area"] == 0.0).all()
    else:
        assert J.abs().min().item() >= RC.CLEAR


@pytest.mark.parametrize("kind", RC.KINDS)
def test_twins_put_the_minimum_and_the_inverted_elements_where_they_say(kind):
    for name in RC.TWIN_NAMES:
        c, r = RC.case(kind, name, True), RC.reference(kind, name, "cauchy")
        low = r["J"].min(dim=1).values                                            # per element, over its points
        inv = r["inverted_mask"].nonzero().flatten()
        if name != "twin_inverted_last":
            # (a): the smallest det F of the valid elements is element 65 536's, alone in block 256, and it stays clear of zero
            valid = low.clone()
            valid[r["inverted_mask"]] = float("inf")
            assert int(valid.argmin()) == RC.LAST == c.meta["min_elem"] and valid.min().item() >= RC.CLEAR
            assert valid[:RC.LAST].min().item() >= valid[RC.LAST].item() + 0.02
        if name == "twin_min_last":
            assert r["inverted"] == 0 and r["min_J"] == low[RC.LAST].item() and int(low.argmin()) // RC.BLOCK == 256
        elif name == "twin_inverted_elsewhere":
            assert (inv // RC.BLOCK).tolist() == [0, 128, 255] and r["inverted"] == 3 and r["min_J"] < 0.0
        else:
            assert (inv // RC.BLOCK).tolist() == [0, 128, 256] and inv[-1].item() == RC.LAST and r["inverted"] == 3
            assert math.isinf(r["eta2"][RC.LAST].item())
    # the last element's share of both totals (eta2 >= 1.0e-7, norm2 >= 1.4e-5) is far above the 1e-12 the device's totals are held to
    r = RC.reference(kind, "ne65537", "cauchy")
    assert r["eta2"][RC.LAST].item() > 1e-8 * r["eta2_total"] and r["norm2"][RC.LAST].item() > 1e-5 * r["norm2_total"]
    for law in RC.LINEAR_LAWS:
        r = RC.reference(kind, "ne65537", law)
        assert r["eta2"][RC.LAST].item() > 1e-8 * r["eta2_total"] and r["norm2"][RC.LAST].item() > 1e-5 * r["norm2_total"]


def test_one_point_pattern_and_the_dead_nodes():
    r = RC.reference("quad4", "one_point", "cauchy")
    np.testing.assert_allclose(r["J"][4].numpy(), RC.ONE_POINT_DET_F, atol=5e-4, rtol=0.0)
    assert (r["J"][4] <= 0.0).sum().item() == 1 and r["inverted_mask"].tolist() == [False] * 4 + [True] + [False] * 4
    assert (r["area"] > 0.0).all()                                                # each of its nodes has valid neighbours
    for kind in RC.KINDS:
        c, r = RC.case(kind, "end_inverted", True), RC.reference(kind, "end_inverted", "cauchy")
        dead, shared = c.meta["dead"], c.meta["shared"]
        assert r["inverted_mask"].tolist() == [False, True]
        assert (r["nodal_stress"][dead] == 0.0).all() and (r["area"][dead] == 0.0).all() and (r["nodal_J"][dead] == 0.0).all()
        # element 0 is a homogeneous stretch diag(1.25, 1.125): the shared nodes carry its one stress and its det F alone
        one = r["sig_h"][0, 0]
        assert (r["nodal_stress"][shared] - one).abs().max().item() <= 1e-14 * one.abs().max().item()
        assert (r["nodal_J"][shared] - 1.25 * 1.125).abs().max().item() <= 1e-15
        assert (r["J"][1] - (-0.8125 if kind == "tri3" else -0.84375)).abs().max().item() <= 1e-14
