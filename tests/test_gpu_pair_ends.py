"""The two ENDS of the paired-slot kernel (tri3_pair.hip) -- the prologue in front of the slot loop (one scalar round trip,
the sum workgroup of a lagged launch told apart after the index loads, accumulators cleared up to their stride under the
first memory round trip) and what follows it (LDS-free wave sum of the tile energy, then the write-out) -- on the smallest
shapes that reach every path they touch:

| case | mesh | why |
|---|---|---|
| a | 6 x 5 nodes, one tile | n_launch = 1; a lagged grid of 2 (the sum workgroup takes tile 0's index); waves with no slot at all |
| b | 41 x 21 nodes, tile_elems 48 | tiles own < 64 nodes and hold < 64 slots: partly filled waves, whole write-out rows masked, 34 tiles (not a multiple of 8) |
| c | 101 x 51 nodes, default tile policy | boundary tiles with edges, 31 tiles (the policy shrinks them to <= 208 owned nodes) |
| d | the mesh of c, plan_pair_block 512 | the <512, 2, 2> instance: eight waves in the reduction |
| e | the mesh of c, tile_elems 950 | tiles own > 512 nodes (538 <= 560): the THIRD write-out / zero-fill row is live in the compile-time-stride instance <256, 3, 3, 4, 560> (the default tile policy shrinks the tiles of a mesh this small: case c does not get there) |
| f | the mesh of c, tile_elems 1040 | the same with 584 owned nodes: the runtime-stride instance, cleared up to cap_owned_rt |

The loss bits are held against tests/golden/pair_ends_parent.npz, recorded by scripts/record_pair_ends.py at the commit before
the rework (the tile energy is documented as bit-reproducible: lane 0's association tree and the wave order are unchanged);
inputs come from that script's build_case, so recorder and test cannot drift apart.  Gradients: the oracle, at
tests/test_gpu_parity.py's tolerances (loss rel 1e-12, gradients max-abs 1e-10 * max|g|)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import record_pair_ends as RP  # noqa: E402

LOSS_RTOL = 1e-12     # tests/test_gpu_parity.py
GRAD_RTOL = 1e-10
NAMES = sorted(RP.CASES)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pair_ends_parent.npz"))


@pytest.fixture(scope="module")
def cases():
    """Every case built once (model + plan), with one plain evaluation and the oracle's numbers, shared and left unchanged."""
    from oracle import closed_form as CF
    out = {}
    for name in NAMES:
        c = RP.build_case(name, _dev())
        c.first = RP.plain_loss(c)
        m = c.model
        coords, conn, geom, bc, _, edges = c.mesh
        X, U = m.coords.detach().cpu().numpy(), m.u_full.detach().cpu().numpy()
        e, gX, gU = CF.tri3_energy(X, U, conn.numpy(), CF.plane_stress(), 0.25)
        e -= CF.edge2_energy(X, U, edges.numpy(), Tconst=np.array([2e5, 0.0, 0.0, 0.0]), gX=gX, gU=gU)
        c.oracle = (e, gX[~geom.numpy()], gU[~bc.numpy()])
        out[name] = c
    return out


def _caller_order(c, res):
    m = c.model
    dev = m.node_coords_free.device
    return (m.to_caller_order(torch.from_numpy(res[1]).to(dev), "x").cpu().numpy(),
            m.to_caller_order(torch.from_numpy(res[2]).to(dev), "u").cpu().numpy())


def _assert_grad_close(got, want, what):
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max()
    assert err <= GRAD_RTOL * scale, f"{what}: max-abs err {err:.3e} vs scale {scale:.3e}"


def test_the_cases_reach_the_paths_they_are_there_for(cases):
    st = {n: cases[n].plan.stats for n in NAMES}
    assert all(cases[n].plan.is_paired() for n in NAMES)
    assert st["a"]["n_tiles"] == 1
    assert st["b"]["max_tile_owned"] < 64 and st["b"]["max_tile_elems"] < 64 and st["b"]["n_tiles"] % 8 != 0
    assert st["c"]["threads_per_tile"] == 256 and st["c"]["max_tile_edges"] > 0 and st["c"]["max_tile_owned"] <= 512
    assert st["d"]["threads_per_tile"] == 512 and st["d"]["slot_rows"] <= 2 and st["d"]["max_tile_nodes"] <= 1024
    assert 512 < st["e"]["max_tile_owned"] <= 560 and st["e"]["max_tile_nodes"] <= 656 and st["e"]["slot_rows"] == 3
    assert 560 < st["f"]["max_tile_owned"] and st["f"]["max_tile_nodes"] <= 768 and st["f"]["slot_rows"] == 3


@pytest.mark.parametrize("name", NAMES)
def test_loss_bits_are_the_parent_commits(cases, golden, name):
    c = cases[name]
    want, want_lag = golden[name + "/loss"][0], golden[name + "/lagged"]
    got, got_lag = c.first[0], RP.lagged_losses(c)
    print(name, "plain", float(got).hex(), float(want).hex(), "lagged", [float(v).hex() for v in got_lag],
          [float(v).hex() for v in want_lag])
    assert np.float64(got).tobytes() == np.float64(want).tobytes(), (name, float(got).hex(), float(want).hex())
    assert got_lag.tobytes() == want_lag.tobytes(), (name, got_lag, want_lag)
    assert want_lag[0] == 0.0 and want_lag[1] == want            # nothing delivered first; then evaluation 1 = the plain one


@pytest.mark.parametrize("name", NAMES)
def test_gradients_match_the_oracle(cases, name):
    c = cases[name]
    e, gX, gU = c.oracle
    assert abs(c.first[0] - e) <= LOSS_RTOL * abs(e), (name, c.first[0], e)
    gx, gu = _caller_order(c, c.first)
    _assert_grad_close(gx, gX, name + " grad_node_coords_free")
    _assert_grad_close(gu, gU, name + " grad_u_free")


@pytest.mark.parametrize("big,small", [("c", "b"), ("e", "a"), ("f", "b")])
def test_no_stale_lds_between_launches_of_different_shapes(cases, big, small):
    """big, then small, then big again in one process: a zero-fill that misses a row shows up in the second evaluation of
    `big` (the issue's sequence is c, b, c; e and f repeat it with the third row live)."""
    first = cases[big].first
    RP.plain_loss(cases[small])
    again = RP.plain_loss(cases[big])
    assert np.float64(again[0]).tobytes() == np.float64(first[0]).tobytes()
    e, gX, gU = cases[big].oracle
    gx, gu = _caller_order(cases[big], again)
    _assert_grad_close(gx, gX, big + " again grad_node_coords_free")
    _assert_grad_close(gu, gU, big + " again grad_u_free")
    fx, fu = _caller_order(cases[big], first)
    _assert_grad_close(gx, fx, big + " again vs first gx")
    _assert_grad_close(gu, fu, big + " again vs first gu")


@pytest.mark.parametrize("name", ["c", "e"])
def test_span_stamps_start_before_the_end(cases, name):
    """The start stamp is now taken unconditionally, in front of the index loads: with a span buffer set, every tile reports a
    non-zero start no later than its end -- also in a lagged launch, whose extra workgroup stamps nothing."""
    import ctypes as C
    from hidenn_fem_amd import _lib
    c = cases[name]
    m, lf, plan = c.model, c.loss_fn, c.plan
    d = m.node_coords_free.device
    L = _lib.lib()
    dv = lambda v: (C.c_double * len(v))(*v)
    _, Tconst = lf._traction(m, None)
    xf, uf, xfix, ufix = m.node_coords_free.detach(), m.u_free.detach(), m.node_coords_fixed, m.u_fixed_rows()
    gx, gu = torch.empty_like(xf), torch.empty_like(uf)
    out = torch.zeros(2, dtype=torch.float64, device=d)
    st = torch.cuda.current_stream().cuda_stream
    nt = plan.n_tiles
    slots = 2
    buf = torch.zeros(slots * nt * 2, dtype=torch.int64, device=d)
    _lib.check(L.hfem_plan_set_span_stamps(plan.handle, buf.data_ptr(), slots))
    try:
        for flags in (8, 8 | 32):                                  # NO_LOSS_SUM, then + SUM_PREVIOUS (grid of nt + 1)
            _lib.check(L.hfem_tri3_energy_plan(plan.handle, xf.data_ptr(), xfix.data_ptr(), uf.data_ptr(), ufix.data_ptr(),
                                               dv(lf._mat), lf._W, dv([0.0] * 6), None, dv(Tconst), 0, -1,
                                               out[1:2].data_ptr(), gx.data_ptr(), gu.data_ptr(), flags, st), "energy")
        torch.cuda.synchronize()
    finally:
        _lib.check(L.hfem_plan_set_span_stamps(plan.handle, None, 0))
    sp = buf.view(slots, nt, 2).cpu().numpy()
    assert (sp[:, :, 0] > 0).all() and (sp[:, :, 1] >= sp[:, :, 0]).all()
    assert out[1].item() == c.first[0]                             # the lagged launch delivered the first one's energy, bit for bit
