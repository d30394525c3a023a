"""The dense mass matrix of tests/modal_reference.py pinned on its own, without a GPU: it is what the mass kernel and the modal
solver are compared against (tests/test_gpu_modal_kernels.py, tests/test_gpu_modal.py)."""
import numpy as np
import pytest

import modal_reference as MR
import zz_reference as Z

MESHES = ["tri_structured", "tri_unstructured", "quad_structured", "quad_split", "quad_split_renumbered"]
_cache = {}


def mesh(name):
    if "meshes" not in _cache:
        _cache["meshes"] = Z.meshes()
    m = _cache["meshes"][name]
    return m[0].numpy(), m[1].numpy()


def dense(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = MR.mass(*mesh(name), **kw)
    return _cache[key]


@pytest.mark.parametrize("name", MESHES)
def test_mass_is_symmetric_positive_definite(name):
    M = dense(name, rho=2.5)
    assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max()
    w = np.linalg.eigvalsh(0.5 * (M + M.T))
    assert w.min() > 1e-6 * w.max()


@pytest.mark.parametrize("lumped", [False, True])
@pytest.mark.parametrize("name", MESHES)
def test_total_mass_is_density_times_area(name, lumped):
    coords, conn = mesh(name)
    M = dense(name, rho=2.5, lumped=lumped)
    one = np.ones(M.shape[0])
    area = MR.total_area(coords, conn)
    assert abs(one @ M @ one - 2.5 * area) <= 1e-13 * 2.5 * area
    # per component of the expanded matrix: a rigid translation in x has no y mass and the other way round
    Me = MR.expand(M)
    ex = np.tile([1.0, 0.0], M.shape[0])
    ey = np.tile([0.0, 1.0], M.shape[0])
    assert abs(ex @ Me @ ex - 2.5 * area) <= 1e-13 * 2.5 * area and abs(ey @ Me @ ey - 2.5 * area) <= 1e-13 * 2.5 * area
    assert ex @ Me @ ey == 0.0


@pytest.mark.parametrize("name", ["tri_structured", "tri_unstructured"])
def test_tri3_closed_form_is_the_quadrature_statement(name):
    coords, conn = mesh(name)
    for nd in conn[::7]:
        a, b = MR.tri3_element(coords[nd], 1.7), MR.tri3_quadrature(coords[nd], 1.7)
        assert np.abs(a - b).max() <= 1e-14 * np.abs(a).max()


@pytest.mark.parametrize("name", ["quad_structured", "quad_split", "quad_split_renumbered"])
def test_quad4_two_point_gauss_is_already_exact(name):
    """The kernel integrates with 2x2 Gauss, the reference with 3x3: N_a N_b |det J| is cubic per variable on a bilinear cell
    (det J keeps its sign inside a valid cell), so both are exact."""
    M3, M2 = dense(name), dense(name, quad_order=2)
    print(name, f"max |M3 - M2| / max |M3| = {np.abs(M3 - M2).max() / np.abs(M3).max():.2e}")
    assert np.abs(M3 - M2).max() <= 1e-14 * np.abs(M3).max()


@pytest.mark.parametrize("name", MESHES)
def test_lumped_is_the_row_sums(name):
    M, Ml = dense(name), dense(name, lumped=True)
    assert np.count_nonzero(Ml - np.diag(np.diag(Ml))) == 0
    assert np.abs(np.diag(Ml) - M.sum(axis=1)).max() <= 1e-15 * np.abs(M).max()
    assert np.diag(Ml).min() > 0.0


def test_free_rows_follow_the_row_order():
    M = dense("tri_structured")
    rows = np.array([5, 2, 9])
    F = MR.free_rows(M, rows)
    assert F.shape == (6, 6)
    assert F[0, 2] == M[5, 2] and F[1, 3] == M[5, 2] and F[0, 3] == 0.0 and F[4, 4] == M[9, 9]
