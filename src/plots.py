from hidenn_fem_amd.post import (StressRecovery, ZZError, compute_du_dx_per_element, node_adjacency, recover_stress,  # noqa: F401
                                 von_mises, zz_error)    # compute cores of src/plots.py + the stress recovery
from hidenn_fem_amd.post import HyperStressRecovery, HyperZZError, hyper_zz_error, recover_cauchy_stress  # noqa: F401
