"""ipm_device.solve_device_genpow: the interior-point loop with the iterate resident in HBM on cone lists that hold
generalized power cones -- the reference's known answer, the mixed-size generator problem and a problem with all seven
cone kinds against ipm.solve over HipSystemBackend (the only device route before), with the criteria of
tests/test_gpu_genpow_ipm.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import ipm, problems
from cuclarabel_amd.cones import ExponentialConeT, ZeroConeT
from cuclarabel_amd.ipm_device import solve_device, solve_device_nonsymmetric, solve_device_genpow
from tests import genpow_reference as G
from tests import nonsymmetric_reference as nr
from tests.golden import genpow_fixtures as F
from tests.test_gpu_ipm_device_nonsym import _resident

pytestmark = pytest.mark.gpu


def _refused(P, q, A, b, cones):
    for fn in (solve_device, solve_device_nonsymmetric):
        with pytest.raises(ValueError):
            fn(P, q, A, b, cones)


@pytest.mark.parametrize("plumbing", ["device", "torch"])
def test_reference_known_answer(plumbing):
    P, q, A, b, cones, exp = F.basic_genpow()
    seen = []
    r = solve_device_genpow(P, q, A, b, cones, inspect=_resident(seen), plumbing=plumbing)
    print("basic_genpow", plumbing, r.status, r.iterations, r.obj_val)
    assert r.status == exp["status"] == ipm.SOLVED
    assert abs(r.obj_val - exp["obj"]) <= F.ATOL
    assert len(seen) >= r.iterations + 1 and min(seen) >= 15
    _refused(P, q, A, b, cones)


def test_generator_problem_against_the_host_loop():
    pb = problems.generalized_power_mix(copies=1)
    seen, kept = [], []

    def inspect(vecs, backend):
        _resident(seen)(vecs, backend)
        kept.append(backend)
    r_dev = solve_device_genpow(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspect)
    be = ipm.HipSystemBackend(pb.P, pb.A, pb.cones)
    r_host = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, be)
    print("device loop", r_dev.status, r_dev.iterations, r_dev.obj_val, "host loop", r_host.status, r_host.iterations, r_host.obj_val)
    assert r_dev.status == ipm.SOLVED and r_host.status == ipm.SOLVED
    assert abs(r_dev.obj_val - r_host.obj_val) <= F.ATOL
    assert kept and kept[0].ks.fallbacks == (0, 0)
    _refused(pb.P, pb.q, pb.A, pb.b, pb.cones)


def test_all_seven_cone_kinds_against_the_host_loop():
    """genpow_reference.mixed_problem over MIXED with an exponential cone added; q and b are chosen so that the problem
    is strictly feasible on both sides: b = A x0 + s0, q = -A'z0 - P x0 at an interior (s0, z0)"""
    specs = G.MIXED[:3] + [ExponentialConeT()] + G.MIXED[3:]
    P, A, s, z = G.mixed_problem(23, specs)
    rng = np.random.default_rng(29)
    off = 0
    for c in specs:
        if isinstance(c, ExponentialConeT):
            s[off:off + 3], z[off:off + 3] = nr.random_interior_pair(c, rng)
        elif isinstance(c, ZeroConeT):
            s[off:off + c.numel] = 0.0
        off += c.numel
    x0 = rng.standard_normal(P.shape[0])
    Pf = P + sp.triu(P, 1).T
    b = A @ x0 + s
    q = -(A.T @ z) - Pf @ x0
    r_dev = solve_device_genpow(P, q, A, b, specs)
    r_host = ipm.solve(P, q, A, b, specs, ipm.HipSystemBackend(P, A, specs))
    print("device loop", r_dev.status, r_dev.iterations, r_dev.obj_val, "host loop", r_host.status, r_host.iterations, r_host.obj_val)
    assert r_dev.status == ipm.SOLVED and r_host.status == ipm.SOLVED
    assert abs(r_dev.obj_val - r_host.obj_val) <= F.ATOL
    _refused(P, q, A, b, specs)
