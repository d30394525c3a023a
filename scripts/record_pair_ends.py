#!/usr/bin/env python3
"""Dev tool (GPU box): the inputs of tests/test_gpu_pair_ends.py and the recorder of its fixture.

    python scripts/record_pair_ends.py [--lib libhidenn_hip_NAME.so] [--out tests/golden/pair_ends_parent.npz]

The fixture holds the LOSS BITS of the paired-slot kernel (tri3_pair.hip) on six small meshes, recorded at the commit
BEFORE the kernel's prologue and reduction were reworked (one scalar round trip, early zero-fill, LDS-free wave sum):
the tile energy is documented as bit-reproducible, so the rework must reproduce every bit.
Re-record only from a commit whose loss bits are the reference (check it out, build, run this script).  The test builds its
inputs through `build_case` / `plain_loss` / `lagged_losses` below, so recorder and test cannot drift apart.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F64 = torch.float64
FIXTURE = os.path.join(ROOT, "tests", "golden", "pair_ends_parent.npz")

# name -> (nx, ny, tile_elems, plan_pair_block or None); why these six: tests/test_gpu_pair_ends.py
CASES = {
    "a": (6, 5, 0, None),
    "b": (41, 21, 48, None),
    "c": (101, 51, 0, None),
    "d": (101, 51, 0, 512),
    "e": (101, 51, 950, None),
    "f": (101, 51, 1040, None),
}


class Case:
    def __init__(self, name, model, loss_fn, plan, mesh):
        self.name, self.model, self.loss_fn, self.plan, self.mesh = name, model, loss_fn, plan, mesh


def build_case(name, device):
    """Mesh (jitter 0.2), u_free ~ 1e-5 N(0, 1) from a fixed seed, Dirichlet / Neumann sets as bench.py's, and the plan."""
    from hidenn_fem_amd import _lib
    from hidenn_fem_amd.loss import EnergyLoss2D
    from hidenn_fem_amd.mesh import structured_tri_mesh
    from hidenn_fem_amd.models import PiecewiseLinearShapeNN2D
    nx, ny, tile_elems, pair_block = CASES[name]
    mesh = structured_tri_mesh(nx, ny, length=2.0, height=1.0, jitter=0.2, seed=0, dtype=F64)
    coords, conn, geom, bc, _, edges = mesh
    torch.manual_seed(0)
    model = PiecewiseLinearShapeNN2D(coords, conn, boundary_mask=geom, dirichlet_mask=bc, u_fixed=0.0, neumann_edges=edges).to(device)
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        model.u_free.copy_((1e-5 * torch.randn(model.u_free.shape, generator=g, dtype=F64)).to(device))
    loss_fn = EnergyLoss2D(E=10e9, nu=0.3, gauss_order=4, device=device, dtype=F64, tile_elems=tile_elems)
    L = _lib.lib()
    prev = L.hfem_get_option(b"plan_pair_block")
    try:
        if pair_block is not None:
            _lib.check(L.hfem_set_option(b"plan_pair_block", pair_block))
        plan = model.tile_plan(tile_elems)               # built here, cached by the model: every later call reuses it
    finally:
        L.hfem_set_option(b"plan_pair_block", prev)
    return Case(name, model, loss_fn, plan, mesh)


def plain_loss(case):
    """One plain evaluation: (loss, gx, gu) as float64 numpy (gradient rows in the model's storage order)."""
    m = case.model
    m.zero_grad()
    loss = case.loss_fn(m)
    loss.backward()
    torch.cuda.synchronize()
    return (np.float64(loss.item()), m.node_coords_free.grad.detach().cpu().numpy().copy(),
            m.u_free.grad.detach().cpu().numpy().copy())


def lagged_losses(case):
    """Three evaluate_local_lagged() calls (u_free scaled by 1.5 between them) + flush_loss(): the loss slot after each of the
    four launches -- 0 (nothing delivered yet), then the energies of evaluations 1, 2, 3."""
    from hidenn_fem_amd.sharded import ShardedTri3Energy
    m = case.model
    keep = m.u_free.detach().clone()
    sh = ShardedTri3Energy(m, case.loss_fn, plan=case.plan, rank=0, world=1)
    out = []
    sh.begin_lagged()
    for k in range(3):
        if k:
            with torch.no_grad():
                m.u_free.mul_(1.5)
        out.append(sh.evaluate_local_lagged().clone())
    out.append(sh.flush_loss().clone())
    torch.cuda.synchronize()
    with torch.no_grad():
        m.u_free.copy_(keep)
    return np.array([v.item() for v in out], dtype=np.float64)


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else FIXTURE
    if "--lib" in argv:
        from hidenn_fem_amd import _lib
        _lib.LIB_PATH = os.path.join(ROOT, "hidenn_fem_amd", "csrc", argv[argv.index("--lib") + 1])
    dev = torch.device("cuda:0")
    rec = {}
    for name in CASES:
        c = build_case(name, dev)
        rec[name + "/loss"] = np.array([plain_loss(c)[0]], dtype=np.float64)
        rec[name + "/lagged"] = lagged_losses(c)
        print(name, c.plan.stats["n_tiles"], rec[name + "/loss"][0].hex(), [float(v).hex() for v in rec[name + "/lagged"]], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()
