"""ipm_device.solve_device_nonsymmetric: the non-symmetric branch of the interior-point loop with the iterate resident in
HBM, on the known-answer fixtures tests/test_gpu_nonsymmetric_ipm.py uses (same criteria as its level-C backends) and on
the entropy-maximisation workload, against ipm.solve over HipSystemBackend."""
import numpy as np
import pytest

from cuclarabel_amd import ipm, problems
from cuclarabel_amd.ipm_device import solve_device, solve_device_nonsymmetric
from tests.golden import nonsymmetric_fixtures as F

pytestmark = pytest.mark.gpu


def _resident(seen):
    """an inspect hook: every vector the loop holds is a device tensor, on every iteration"""
    import torch

    def inspect(vecs, backend):
        for name, t in vecs.items():
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64, name
        seen.append(len(vecs))
    return inspect


@pytest.mark.parametrize("plumbing", ["device", "torch"])
@pytest.mark.parametrize("fixture", [F.basic_exp, F.basic_pow], ids=lambda f: f.__name__)
def test_reference_known_answers(fixture, plumbing):
    P, q, A, b, cones, exp = fixture()
    seen = []
    r = solve_device_nonsymmetric(P, q, A, b, cones, inspect=_resident(seen), plumbing=plumbing)
    print(fixture.__name__, plumbing, r.status, r.iterations, r.obj_val)
    assert r.status == exp["status"] == ipm.SOLVED
    if exp["x"] is not None:
        assert np.linalg.norm(r.x - exp["x"]) <= F.ATOL
    assert abs(r.obj_val - exp["obj"]) <= F.ATOL
    assert len(seen) >= r.iterations + 1 and min(seen) >= 15
    with pytest.raises(ValueError, match="solve_device_nonsymmetric"):
        solve_device(P, q, A, b, cones)


def test_entropy_maximisation_with_64_cones_against_the_host_loop():
    pb = problems.entropy_maximization(64)
    seen = []
    r_dev = solve_device_nonsymmetric(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=_resident(seen))
    be = ipm.HipSystemBackend(pb.P, pb.A, pb.cones)
    r_host = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, be)
    print("device loop", r_dev.status, r_dev.iterations, r_dev.obj_val, "host loop", r_host.status, r_host.iterations, r_host.obj_val)
    assert r_dev.status == ipm.SOLVED and r_host.status == ipm.SOLVED
    # both stop at the 1e-8 gap tolerance; the feasibility residuals enter the objective too: 100 x that
    # (the criterion of test_entropy_maximisation_with_20000_cones_device_against_cpu)
    assert abs(r_dev.obj_val - r_host.obj_val) <= 1e-6 * max(1.0, abs(r_host.obj_val))
    assert seen
    with pytest.raises(ValueError, match="solve_device_nonsymmetric"):
        solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones)


def test_generalized_power_cones_are_refused():
    import scipy.sparse as sp
    from cuclarabel_amd.cones import GenPowerConeT, NonnegativeConeT
    with pytest.raises(ValueError):
        solve_device_nonsymmetric(sp.identity(4, format="csc"), np.zeros(4), sp.identity(4, format="csc"), np.ones(4),
                                  [NonnegativeConeT(1), GenPowerConeT((0.5, 0.5), 1)])
