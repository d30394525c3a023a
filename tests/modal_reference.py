"""Dense numpy statement of the mass matrix of a TRI3 or QUAD4 mesh, shared by the modal tests (a plain helper
module, not a conftest), built element by element and independent of the kernel's formulas:

    M_e[a][b] = rho int_e N_a N_b dA
    TRI3:  the closed form rho |det J| / 24 (1 + delta_ab)   (``tri3_quadrature`` states the same by a degree-2 rule)
    QUAD4: 3x3 Gauss (the kernel uses 2x2, which is already exact for a bilinear cell; ``order=2`` gives that rule)
    lumped: the row sums on the diagonal

``M`` is scalar [Nn, Nn] over the nodes; it acts per displacement component (M x I_2).  ``expand`` / ``free_rows`` give the
[2 n_u, 2 n_u] matrix over the free u rows in a given row order, interleaved (x, y) per row as ``u_free`` is.
"""
import numpy as np

XI = np.array([-1.0, 1.0, 1.0, -1.0])
ETA = np.array([-1.0, -1.0, 1.0, 1.0])


def gauss(order):
    x, w = np.polynomial.legendre.leggauss(order)
    return x, w


def tri3_element(xe, rho=1.0):
    """[3, 3] closed form; xe [3, 2]."""
    det = (xe[1, 0] - xe[0, 0]) * (xe[2, 1] - xe[0, 1]) - (xe[2, 0] - xe[0, 0]) * (xe[1, 1] - xe[0, 1])
    return rho * abs(det) / 24.0 * (np.ones((3, 3)) + np.eye(3))


def tri3_quadrature(xe, rho=1.0):
    """The same by the 3-point edge-midpoint rule (exact for degree 2): N = (xi, eta, 1 - xi - eta)."""
    det = (xe[1, 0] - xe[0, 0]) * (xe[2, 1] - xe[0, 1]) - (xe[2, 0] - xe[0, 0]) * (xe[1, 1] - xe[0, 1])
    pts = np.array([[0.5, 0.0], [0.5, 0.5], [0.0, 0.5]])
    m = np.zeros((3, 3))
    for xi, eta in pts:
        N = np.array([xi, eta, 1.0 - xi - eta])
        m += (abs(det) / 6.0) * np.outer(N, N)
    return rho * m


def quad4_element(xe, rho=1.0, order=3):
    """[4, 4] by order x order Gauss; xe [4, 2], local nodes at (-1,-1), (1,-1), (1,1), (-1,1)."""
    x, w = gauss(order)
    m = np.zeros((4, 4))
    for xi, wx in zip(x, w):
        for eta, wy in zip(x, w):
            N = 0.25 * (1 + XI * xi) * (1 + ETA * eta)
            dxi = 0.25 * XI * (1 + ETA * eta)
            deta = 0.25 * ETA * (1 + XI * xi)
            J = np.array([[dxi @ xe[:, 0], deta @ xe[:, 0]], [dxi @ xe[:, 1], deta @ xe[:, 1]]])
            m += wx * wy * abs(np.linalg.det(J)) * np.outer(N, N)
    return rho * m


def element_area(xe):
    """Area of a TRI3 or QUAD4 element (shoelace; the orientation does not matter)."""
    x, y = xe[:, 0], xe[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def mass(coords, conn, rho=1.0, lumped=False, quad_order=3):
    """Scalar mass matrix [Nn, Nn] over the nodes (dense)."""
    coords, conn = np.asarray(coords, dtype=np.float64), np.asarray(conn, dtype=np.int64)
    nn, npe = coords.shape[0], conn.shape[1]
    M = np.zeros((nn, nn))
    for e in range(conn.shape[0]):
        nd = conn[e]
        me = tri3_element(coords[nd], rho) if npe == 3 else quad4_element(coords[nd], rho, quad_order)
        M[np.ix_(nd, nd)] += me
    if lumped:
        M = np.diag(M.sum(axis=1))
    return M


def total_area(coords, conn):
    coords, conn = np.asarray(coords, dtype=np.float64), np.asarray(conn, dtype=np.int64)
    return sum(element_area(coords[nd]) for nd in conn)


def expand(M):
    """M x I_2: [2 n, 2 n] acting on rows interleaved (x, y)."""
    return np.kron(M, np.eye(2))


def free_rows(M, row_node):
    """The [2 n_u, 2 n_u] matrix over the free u rows: ``row_node[r]`` = node id of row r (Dirichlet nodes are simply absent)."""
    row_node = np.asarray(row_node, dtype=np.int64)
    return expand(M[np.ix_(row_node, row_node)])
