"""The line search of the QUAD4 r-adaptive loop on fp32 coordinate rows, without a GPU.  The step bound holds for ``x + alpha d``; the
rows hold that rounded to float.  On a cell a few float spacings wide the rounding alone takes it below ``eta``, so the line search
measures the rounded trial against the rows it started from and halves a trial that keeps less than ``eta`` -- where the mesh
class asks for it (QUAD4; fp64 rows and the TRI3 solver are not measured).  The loop is run
here on one hand-built cell, with the numpy closed forms of tests/test_radapt_quad4_host.py in place of the mesh kernels."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from test_radapt_quad4_host import quad4_measure_np, quad4_step_bound_np

ULP = 2.0 ** -23                                      # the float spacing in [1, 2)


class _OneCellMesh:
    """What ``_line_search`` asks of a mesh, for one cell whose corner rows are the model's four rows."""

    def __init__(self, model, f32, measure_f32_trials):
        self.model, self.f32, self.measure_f32_trials, self.measured = model, f32, measure_f32_trials, 0

    def rows(self):
        return self.model.node_coords_free.detach().double().numpy().reshape(1, 4, 2)

    def step_bound(self, d, eta):
        return torch.tensor(quad4_step_bound_np(self.rows(), d.numpy().reshape(1, 4, 2), eta)[0].min())

    def measure(self, x_ref=None, per_element=True):
        self.measured += 1
        q, r, inv = quad4_measure_np(self.rows(), x_ref.double().numpy().reshape(1, 4, 2))
        return None, None, torch.tensor([q.min(), r.min(), float(inv.sum())], dtype=torch.float64)


def _search(dtype, mesh_cls=None):
    from hidenn_fem_amd import radapt
    mesh_cls = mesh_cls or radapt._QuadMesh
    # a cell five float spacings wide; the direction closes it from both sides
    x = torch.tensor([[1.0, 0.0], [1.0 + 5 * ULP, 0.0], [1.0 + 5 * ULP, 1.0], [1.0, 1.0]], dtype=torch.float64)
    d = torch.tensor([[1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]], dtype=torch.float64).reshape(-1)
    model = SimpleNamespace(node_coords_free=x.to(dtype).clone())
    assert torch.equal(model.node_coords_free.double(), x)            # the rows are float numbers
    s = object.__new__(radapt.Quad4RAdaptiveSolver)
    s.model, s.mesh = model, _OneCellMesh(model, dtype == torch.float32, mesh_cls.measure_f32_trials)
    s.eta, s.max_ls, s.c1 = 0.25, 20, 1e-4
    evaluated = []

    def objective():                                                  # the cell's width: falls along d
        evaluated.append(model.node_coords_free.detach().double().clone())
        return float(evaluated[-1][1, 0] - evaluated[-1][0, 0])

    s.objective = objective
    x0 = x.reshape(-1).clone()
    alpha, amax, f, trials = s._line_search(x0, d, 5 * ULP, -2.0, math.inf, x.to(dtype))
    return s, x, alpha, amax, trials, evaluated


def test_an_fp32_trial_that_rounding_collapses_is_halved_before_the_energy_is_evaluated():
    s, x, alpha, amax, trials, evaluated = _search(torch.float32)
    assert amax == 1.875 * ULP                                        # c_k is linear along d: eta = 0.25 is kept up to 3/4
    # 0.9 amax puts the sides at 1.6875 and 3.3125 spacings (width 0.325 of 5), which round to 2 and 3: width 0.2 of 5.  That
    # trial is measured, not evaluated, and halved: 0.84375 and 4.15625 round to 1 and 4, width 0.6 of 5
    assert trials == 2 and alpha == 0.45 * amax and s.mesh.measured == 2 and len(evaluated) == 1
    rows = s.model.node_coords_free.double().numpy().reshape(1, 4, 2)
    _, ratio, inverted = quad4_measure_np(rows, x.numpy().reshape(1, 4, 2))
    assert ratio.min() == 0.6 and not inverted.any()
    assert np.all(quad4_measure_np(evaluated[0].numpy().reshape(1, 4, 2), x.numpy().reshape(1, 4, 2))[1] >= 0.25)


def test_an_fp64_trial_is_not_measured():
    s, x, alpha, amax, trials, evaluated = _search(torch.float64)
    assert amax == 1.875 * ULP and trials == 1 and alpha == 0.9 * amax and s.mesh.measured == 0 and len(evaluated) == 1
    rows = s.model.node_coords_free.numpy().reshape(1, 4, 2)
    ratio = quad4_measure_np(rows, x.numpy().reshape(1, 4, 2))[1].min()
    assert abs(ratio - 0.325) <= 1e-9                                 # 1 - 0.9 * 0.75, up to the rounding of the two sums


def test_the_tri3_mesh_class_leaves_fp32_trials_unmeasured_as_before():
    from hidenn_fem_amd import radapt
    assert radapt.RAdaptiveSolver._mesh_cls is radapt._Mesh and radapt.Quad4RAdaptiveSolver._mesh_cls is radapt._QuadMesh
    s, x, alpha, amax, trials, evaluated = _search(torch.float32, radapt._Mesh)
    assert trials == 1 and alpha == 0.9 * amax and s.mesh.measured == 0 and len(evaluated) == 1
