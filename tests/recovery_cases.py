"""Cases at the size, valence and inversion edges of the recovery kernels (csrc/recover.hip: stress_recover_kernel,
zz_error_kernel, zz_finish_kernel), shared by tests/test_recovery_cases_host.py and tests/test_gpu_recovery_edges.py (a plain
helper module, not a conftest; of the library only ``hidenn_fem_amd.post.node_adjacency`` and ``hidenn_fem_amd.mesh``, both CPU).

A case is ``Case(coords [nn, 2], u [nn, 2], conn [ne, npe], meta)``, deterministic fp64 on the CPU, for the raw C ABI (no model,
no plan).  ``case(kind, name, finite)``: kind "tri3" | "quad4"; ``finite`` picks the displacement, ``hyper_zz_reference.field``
for the Cauchy law and ``zz_reference.field`` for the two linear laws.  Expected results are ``reference(kind, name, law)`` =
``zz_reference.zz`` / ``hyper_zz_reference.zz`` as they are (C = ``plane_stress_C()``, (lambda, mu) = ``lame()``); nothing of the
kernels' formulas is restated here.

Names (sizes from csrc/recover.hip: 256 threads per block, one thread per node / per element, one partial per block, the finish
kernel's thread t adds partials t, t + 256, ...):

  ne1 ... ne65537      the first ne elements of one jittered structured mesh with 65 792 of them; the nodes that no kept element
                       references stay in ``coords`` (their rows come out zero).  65 536 -> 256 partials, 65 537 -> 257: the
                       finish kernel's thread 0 makes a second trip whose only partial is that of element 65 536 alone.
  patch257, patch65537 ``zz_reference.linear_field`` on ne257 / ne65537 (linear laws, physical convention: eta = 0)
  nn255, nn256, nn257  every node referenced: a zigzag triangle strip; a two-row cell strip, for the odd counts with one more cell
                       that shares a single corner with it.  nn257_orphan: 256 such nodes and a last one of no element.
  fan3, fan_big        a closed fan around a hub (node 0): 3 elements, and 300 triangles / 64 cells; element i lists the hub at
                       local corner i mod npe; the ring radii are modulated, so no two elements are congruent.
  finite strain only:
  twin_min_last        ne65537 with one node of element 65 536 moved so that this element holds the smallest det F of all
                       (>= 0.05): the minimum sits in the partial of the second trip.
  twin_inverted_elsewhere   the same, and three elements inverted: one in block 0, one in block 128, one in block 255
  twin_inverted_last   three elements inverted: one in block 0, one in block 128, and element 65 536
  det_zero             one element with det F == 0.0 exactly (the boundary of the rule j > -1): collapsed onto an edge
  one_point            (quad4) a 3 x 3 patch of unit cells, corner 2 of the centre cell displaced by (-0.7, -0.7): det F =
                       (0.704, 0.300, 0.300, -0.104) at its points -- one point inverted, so the cell is
  end_inverted         two elements; the end one is mirrored (det F = -0.8125 / -0.84375), the other is stretched by
                       diag(1.25, 1.125): the end nodes have only an inverted element, the shared ones the valid one alone

Every det F outside det_zero stays ``CLEAR`` = 0.05 away from zero (tests/test_recovery_cases_host.py asserts it): the device's
j = tr H + det H and the reference's det(F) round differently, and a case near the boundary would test luck.
"""
import collections
import functools
import math

import torch

import hyper_reference as H
import hyper_zz_reference as HZ
import zz_reference as Z
from oracle import ref_chain as R

F64 = torch.float64
BLOCK = 256                                     # kRecBlock
GUARD = 64                                      # doubles of sentinel past every output of the GPU test
CLEAR = 0.05
KINDS = ("tri3", "quad4")
NPE = {"tri3": 3, "quad4": 4}
LINEAR_LAWS = ("reference", "physical")         # LinearLaw<false>, LinearLaw<true>
LAWS = LINEAR_LAWS + ("cauchy",)
LAM, MU = H.lame()

NE_COUNTS = (1, 255, 256, 257, 65536, 65537)
NN_COUNTS = (255, 256, 257)
NE_BIG = 65537
LAST = NE_BIG - 1                               # element 65 536: alone in block 256
FAN_BIG = {"tri3": 300, "quad4": 64}
INVERT_BLOCKS = (0, 128, 255)                   # variant 1; variant 2 swaps the last for block 256 (element LAST)

NE_NAMES = tuple(f"ne{n}" for n in NE_COUNTS)
NN_NAMES = tuple(f"nn{n}" for n in NN_COUNTS) + ("nn257_orphan",)
FAN_NAMES = ("fan3", "fan_big")
PATCH_NAMES = ("patch257", "patch65537")
TWIN_NAMES = ("twin_min_last", "twin_inverted_elsewhere", "twin_inverted_last")
COMMON_NAMES = NE_NAMES + NN_NAMES + FAN_NAMES           # every law


def inversion_names(kind):
    return ("det_zero", "end_inverted") + (("one_point",) if kind == "quad4" else ())


def finite_names(kind):
    return COMMON_NAMES + TWIN_NAMES + inversion_names(kind)


def names(kind, law):
    """The cases a law runs on."""
    if law == "cauchy":
        return finite_names(kind)
    return COMMON_NAMES + (PATCH_NAMES if law == "physical" else ())


def is_patch(kind, name):
    """sigma* = sigma_h up to rounding in every valid element (a linear field; one triangle, whose sigma_h is one constant;
    end_inverted, whose one valid element is a homogeneous stretch): eta of the valid elements is judged by
    ``sqrt(eta^2 / (|u_h|^2 + eta^2)) <= 1e-12``, never by a ratio against a rounding-size eta2."""
    return name in PATCH_NAMES or (kind == "tri3" and name == "ne1") or name == "end_inverted"


Case = collections.namedtuple("Case", "coords u conn meta")


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def t(rows, dtype=F64):
    return torch.tensor(rows, dtype=dtype)


# ---------------------------------------------------------------------------------------------------- geometry
@functools.lru_cache(maxsize=None)
def count_mesh(kind):
    """(coords, conn) of the mesh the element-count cases cut their first ne elements from: 65 792 elements."""
    from hidenn_fem_amd.mesh import structured_quad_mesh, structured_tri_mesh
    if kind == "tri3":
        m = structured_tri_mesh(258, 129, jitter=0.3, seed=6, flip_fraction=0.4, dtype=F64)
    else:
        m = structured_quad_mesh(258, 257, jitter=0.3, seed=3, dtype=F64)
    return m[0], m[1]


def strip(kind, nn, orphan=False):
    """Every one of the nn nodes referenced (``orphan``: one more node, of no element, after them)."""
    if kind == "tri3":
        i = torch.arange(nn, dtype=F64)
        coords = torch.stack([2.0 * i / (nn - 1), 0.5 + 0.02 * (i % 2) + 0.003 * torch.sin(0.37 * i)], dim=1)
        conn = torch.stack([torch.arange(nn - 2) + k for k in range(3)], dim=1)
    else:
        k = (nn - (nn % 2) * 3) // 2                               # 2k nodes in the strip, + 3 of the extra cell when nn is odd
        i = torch.arange(k, dtype=F64)
        x = 2.0 * i / k
        bottom = torch.stack([x, 0.45 + 0.004 * torch.sin(0.53 * i)], dim=1)
        top = torch.stack([x + 0.003 * torch.cos(0.41 * i), 0.47 + 0.004 * torch.sin(0.29 * i + 1.0)], dim=1)
        coords = torch.stack([bottom, top], dim=1).reshape(2 * k, 2)   # bottom i -> node 2i, top i -> node 2i + 1
        j = 2 * torch.arange(k - 1)
        conn = torch.stack([j, j + 2, j + 3, j + 1], dim=1)
        if nn % 2:                                                  # shares the strip's last top node, and nothing else
            a = coords[2 * k - 1]
            coords = torch.cat([coords, a + t([[0.017, 0.002], [0.019, 0.021], [0.001, 0.018]])])
            conn = torch.cat([conn, t([[2 * k - 1, 2 * k, 2 * k + 1, 2 * k + 2]], torch.long)])
        conn = torch.stack([conn[e].roll(-(e % 4)) for e in range(conn.shape[0])])   # the listing starts at corner e mod 4
    if orphan:
        coords = torch.cat([coords, t([[9.0, 9.0]])])
    assert coords.shape[0] == nn + int(orphan)
    return coords, conn


def fan(kind, n):
    """A closed fan of n elements around the hub, node 0 at (1, 0.5); element i lists the hub at local corner i mod npe."""
    npe = NPE[kind]
    i = torch.arange(n, dtype=F64)
    th = 2.0 * math.pi * i / n
    hub = t([[1.0, 0.5]])

    def ring(r, angle):
        return hub + r[:, None] * torch.stack([torch.cos(angle), torch.sin(angle)], dim=1)

    ids = torch.arange(n)
    if kind == "tri3":
        coords = torch.cat([hub, ring(0.35 * (1.0 + 0.2 * torch.sin(2.0 * th + 0.4) + 0.05 * torch.sin(5.0 * th)), th)])
        conn = torch.stack([torch.zeros(n, dtype=torch.long), 1 + ids, 1 + (ids + 1) % n], dim=1)
    else:
        spokes = ring(0.25 * (1.0 + 0.15 * torch.sin(1.3 * i + 0.4)), th)
        outer = ring(0.40 * (1.0 + 0.10 * torch.cos(0.9 * i)), th + math.pi / n)
        coords = torch.cat([hub, spokes, outer])
        conn = torch.stack([torch.zeros(n, dtype=torch.long), 1 + ids, 1 + n + ids, 1 + (ids + 1) % n], dim=1)
    conn = torch.stack([conn[e].roll(e % npe) for e in range(n)])
    return coords, conn


def field(coords, finite):
    return HZ.field(coords) if finite else Z.field(coords)


# ---------------------------------------------------------------------------------------------------- moved nodes
def det_F(coords, u, conn):
    """det F [Ne, NQ] at the element points, by the reference's own ``deformation_gradients``."""
    return torch.linalg.det(HZ.deformation_gradients(coords, u, conn)[0])


SCAN = tuple(0.30 + 0.05 * k for k in range(25))                     # 0.30 ... 1.50
KEEP = 0.3


def push(coords, u, conn, e, goal, ceiling=None):
    """A copy of ``u`` with one node of element e moved, in the deformed configuration, towards the opposite edge (TRI3: its
    foot) or the opposite corner (QUAD4) by the first fraction of ``SCAN``, over the corners in order, at which

    goal "compress": min det F of e lies in [CLEAR + 0.01, ceiling - 0.03] and every other element at that node stays 0.02 above it;
    goal "invert":   min det F of e is <= -(CLEAR + 0.01), no point of an element at that node has |det F| < CLEAR + 0.01, and
                     every other element at that node keeps det F >= KEEP = 0.3, above what "compress" leaves in its element.

    None if there is no such move.  Only the elements at the moved node change, so only they are evaluated."""
    npe = conn.shape[1]
    x = coords + u
    for c in range(npe):
        n = int(conn[e, c])
        if npe == 3:
            p, q = x[conn[e, (c + 1) % 3]], x[conn[e, (c + 2) % 3]]
            target = p + (q - p) * ((x[n] - p) @ (q - p)) / ((q - p) @ (q - p))
        else:
            target = x[conn[e, (c + 2) % 4]]
        near = (conn == n).any(dim=1).nonzero().flatten()
        mine = near == e
        for s in SCAN:
            v = u.clone()
            v[n] = u[n] + s * (target - x[n])
            J = det_F(coords, v, conn[near])
            low, others = J[mine].min().item(), J[~mine]
            rest = others.min().item() if others.numel() else float("inf")
            if goal == "compress":
                ok = CLEAR + 0.01 <= low <= ceiling - 0.03 and rest >= low + 0.02
            else:
                ok = low <= -(CLEAR + 0.01) and J.abs().min().item() >= CLEAR + 0.01 and rest >= KEEP
            if ok:
                return v
    return None


def invert_in_block(coords, u, conn, block):
    """-> (u, e): the first element from the 10th of ``block`` on that ``push`` can invert alone."""
    first = block * BLOCK
    for e in range(first + min(10, conn.shape[0] - 1 - first), min(first + BLOCK, conn.shape[0])):
        v = push(coords, u, conn, e, "invert")
        if v is not None:
            return v, e
    raise RuntimeError(f"no single-element inversion found in block {block}")


@functools.lru_cache(maxsize=None)
def _twin(kind, name):
    coords, conn = count_mesh(kind)
    conn = conn[:NE_BIG]
    u = HZ.field(coords)
    inverted = []
    if name != "twin_inverted_last":
        floor = det_F(coords, u, conn[:LAST]).min().item()           # the smallest det F of the other elements
        u = push(coords, u, conn, LAST, "compress", ceiling=floor)
        assert u is not None, "element 65 536 cannot be made the minimum"
    for block in INVERT_BLOCKS[:2] if name == "twin_inverted_last" else INVERT_BLOCKS if name == "twin_inverted_elsewhere" else ():
        u, e = invert_in_block(coords, u, conn, block)
        inverted.append(e)
    if name == "twin_inverted_last":
        u = push(coords, u, conn, LAST, "invert")
        assert u is not None, "element 65 536 cannot be inverted alone"
        inverted.append(LAST)
    return Case(coords, u, conn, dict(inverted=inverted, min_elem=None if name == "twin_inverted_last" else LAST))


# ---------------------------------------------------------------------------------------------------- hand-written elements
def _det_zero(kind):
    if kind == "tri3":
        return Case(t([[0, 0], [1, 0], [0, 1]]), t([[0, 0], [0, 0], [0, -1]]), t([[0, 1, 2]], torch.long), dict(inverted=[0]))
    return Case(t([[0, 0], [1, 0], [1, 1], [0, 1]]), t([[0, 0], [0, 0], [0, -1], [0, -1]]), t([[0, 1, 2, 3]], torch.long),
                dict(inverted=[0]))


ONE_POINT_DET_F = (0.704, 0.300, 0.300, -0.104)                      # the centre cell's four points, to 5e-4


def _one_point():
    g = torch.arange(4, dtype=F64)
    coords = torch.stack(torch.meshgrid(g, g, indexing="ij"), dim=2).reshape(16, 2)       # node 4 i + j at (i, j)
    cells = [[4 * i + j, 4 * (i + 1) + j, 4 * (i + 1) + j + 1, 4 * i + j + 1] for i in range(3) for j in range(3)]
    u = torch.zeros(16, 2, dtype=F64)
    u[10] = t([-0.7, -0.7])                                            # corner 2 of cell 4 = node (2, 2)
    return Case(coords, u, t(cells, torch.long), dict(inverted=[4]))


def _end_inverted(kind):
    """Element 0 stretched by diag(1.25, 1.125); element 1 mirrored.  ``dead``: the nodes of element 1 alone."""
    if kind == "tri3":
        return Case(t([[0, 0], [1, 0], [0, 1], [1, 1]]), t([[0, 0], [0.25, 0], [0, 0.125], [-0.75, -0.75]]),
                    t([[0, 1, 2], [1, 3, 2]], torch.long), dict(inverted=[1], dead=[3], shared=[1, 2]))
    return Case(t([[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]]),
                t([[0, 0], [0.25, 0], [-1.5, 0], [0, 0.125], [0.25, 0.125], [-1.5, 0.125]]),
                t([[0, 1, 4, 3], [1, 2, 5, 4]], torch.long), dict(inverted=[1], dead=[2, 5], shared=[1, 4]))


# ---------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def case(kind, name, finite):
    """-> Case; ``meta``: inverted (element ids, ascending by construction), and per family hub / dead / shared / min_elem."""
    if name in TWIN_NAMES or name in ("det_zero", "one_point", "end_inverted"):
        assert finite and name in finite_names(kind), (kind, name)
        if name in TWIN_NAMES:
            return _twin(kind, name)
        return _det_zero(kind) if name == "det_zero" else _one_point() if name == "one_point" else _end_inverted(kind)
    meta = dict(inverted=[])
    if name.startswith("ne") or name in PATCH_NAMES:
        coords, conn = count_mesh(kind)
        conn = conn[:int(name[2:] if name.startswith("ne") else name[5:])]
    elif name.startswith("nn"):
        coords, conn = strip(kind, 256 if name.endswith("orphan") else int(name[2:]), orphan=name.endswith("orphan"))
    elif name in FAN_NAMES:
        coords, conn = fan(kind, 3 if name == "fan3" else FAN_BIG[kind])
        meta["hub"] = 0
    else:
        raise KeyError(name)
    if name in PATCH_NAMES:
        assert not finite
        return Case(coords, Z.linear_field(coords), conn, meta)
    return Case(coords, field(coords, finite), conn, meta)


def referenced(c):
    """bool [nn]: the nodes some element lists."""
    mask = torch.zeros(c.coords.shape[0], dtype=torch.bool)
    mask[c.conn.reshape(-1)] = True
    return mask


def adjacency(c):
    from hidenn_fem_amd.post import node_adjacency
    return node_adjacency(c.conn, c.coords.shape[0])


@functools.lru_cache(maxsize=None)
def reference(kind, name, law):
    """The CPU statement of one (case, law): computed once, shared, never modified.  Keys as ``hyper_zz_reference.zz``; the linear
    laws carry nodal_stress, area, eta2, norm2, eta2_total, norm2_total, eta, relative."""
    c = case(kind, name, law == "cauchy")
    if law == "cauchy":
        return HZ.zz(c.coords, c.u, c.conn, LAM, MU)
    Cm = R.plane_stress_C()
    sig, area = Z.recover(c.coords, c.u, c.conn, Cm, law)
    r = Z.zz(c.coords, c.u, c.conn, Cm, law, sig_star=sig)
    r["area"] = area
    return r
