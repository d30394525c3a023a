"""QUAD4 meshes that are not a structured grid (numpy only; a plain helper module, not a conftest).

``split_tri_quads``: every triangle of the Delaunay mesh with holes (``hidenn_fem_amd.mesh.unstructured_tri_mesh``) split into
three quadrilaterals, so the node valence runs from 1 to 11 instead of the structured grid's 4.  ``renumber``: the same mesh in
another numbering -- cell order, node ids, each cell's starting corner and its orientation.  Both return the 6-tuple the
meshers of ``hidenn_fem_amd.mesh`` return."""
import numpy as np
import torch


def split_tri_quads(n_points=700, seed=2, dtype=torch.float64):
    """Each triangle (a, b, c) becomes the quads (vertex, midpoint of the next edge, centroid, midpoint of the previous edge):
    (a, m_ab, g, m_ca), (b, m_bc, g, m_ab), (c, m_ca, g, m_bc).  The triangles are counter-clockwise, and a vertex, the two
    midpoints next to it and the centroid are the corners of a convex kite, so every quad is convex and counter-clockwise.
    Nodes: the triangle vertices, then one per edge, then one per triangle.  A midpoint is boundary / Dirichlet / Neumann iff
    both ends of its edge are; centroids never are.  Each Neumann edge (i, j) becomes (i, m) and (m, j)."""
    from hidenn_fem_amd.mesh import unstructured_tri_mesh
    pts, tri, geom, bc, mn, edges = (t.numpy() for t in unstructured_tri_mesh(n_points, seed=seed, dtype=torch.float64))
    nv, nt = len(pts), len(tri)
    e_all = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    uniq, inv = np.unique(e_all, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    mid = nv + inv.reshape(3, nt).T                                  # [nt, 3]: midpoint node of edge ab, bc, ca
    cen = nv + len(uniq) + np.arange(nt)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    cells = np.concatenate([np.stack([a, mid[:, 0], cen, mid[:, 2]], 1), np.stack([b, mid[:, 1], cen, mid[:, 0]], 1),
                            np.stack([c, mid[:, 2], cen, mid[:, 1]], 1)]).astype(np.int64)
    coords = np.concatenate([pts, 0.5 * (pts[uniq[:, 0]] + pts[uniq[:, 1]]), pts[tri].mean(axis=1)])
    both = lambda m: np.concatenate([m, m[uniq].all(axis=1), np.zeros(nt, dtype=bool)])
    lookup = {(int(i), int(j)): nv + k for k, (i, j) in enumerate(uniq)}
    ed = [[(i, lookup[(min(i, j), max(i, j))]), (lookup[(min(i, j), max(i, j))], j)] for i, j in edges.tolist()]
    ed = np.asarray(ed, dtype=np.int64).reshape(-1, 2)
    return (torch.tensor(coords, dtype=dtype), torch.tensor(cells), torch.tensor(both(geom)), torch.tensor(both(bc)),
            torch.tensor(both(mn)), torch.tensor(ed))


def renumber(mesh, seed, cells=True, nodes=True, rotate=True, orient="ccw"):
    """The same mesh, numbered differently: a random permutation of the cell order (``cells``), a random renumbering of the
    nodes applied to coordinates, masks, connectivity and edges alike (``nodes``), an independent random cyclic rotation
    (0..3) of each cell's corners (``rotate``), and every cell (``orient="cw"``) or a random half of them (``"mixed"``)
    reversed (``[:, [0, 3, 2, 1]]``).  An edge keeps its (i, j) direction: the traction work is not symmetric in the two.
    Returns ``(mesh6, old_of_new)``: node ``k`` of the new mesh is node ``old_of_new[k]`` of the old one, so a per-node array
    ``a_new`` comes back to the old numbering as ``a_old[old_of_new] = a_new``."""
    if orient not in ("ccw", "cw", "mixed"):
        raise ValueError(orient)
    coords, conn, geom, bc, mn, edges = mesh
    rng = np.random.default_rng(seed)
    cn = conn.numpy().copy()
    nn, ne = coords.shape[0], cn.shape[0]
    if cells:
        cn = cn[rng.permutation(ne)]
    new_of_old = rng.permutation(nn) if nodes else np.arange(nn)
    old_of_new = np.argsort(new_of_old)
    cn = new_of_old[cn]
    if rotate:
        cn = np.take_along_axis(cn, (np.arange(4)[None, :] + rng.integers(0, 4, size=ne)[:, None]) % 4, axis=1)
    if orient != "ccw":
        flip = np.ones(ne, dtype=bool) if orient == "cw" else rng.permutation(ne) < ne // 2
        cn[flip] = cn[flip][:, [0, 3, 2, 1]]
    idx = torch.from_numpy(old_of_new)
    ed = torch.from_numpy(new_of_old[edges.numpy()].reshape(-1, 2))
    return (coords[idx], torch.from_numpy(np.ascontiguousarray(cn)), geom[idx], bc[idx], mn[idx], ed), idx


def valence(conn, n_nodes):
    """Number of cells at every node."""
    return np.bincount(np.asarray(conn).reshape(-1), minlength=n_nodes)
