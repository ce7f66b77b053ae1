"""Problems with generalized power cones through the device backends of tests/test_gpu_nonsymmetric_ipm.py's list: the
reference's known answer and the mixed-size generator problem against the CPU run (the scipy backend on the numpy
restatement of the expanded K)."""
import numpy as np
import pytest

from cuclarabel_amd import _lib, ipm, problems
from tests import genpow_reference as G
from tests.golden import genpow_fixtures as F

pytestmark = pytest.mark.gpu

DEVICE_SCALED = ["level_b", "level_c", "level_c_lazy", "level_c_batched"]


def _backend(name, P, A, cones):
    return {"level_b": lambda: ipm.HipBackend(P, A, cones),
            "level_c": lambda: ipm.HipSystemBackend(P, A, cones),
            "level_c_lazy": lambda: ipm.HipSystemBackend(P, A, cones, lazy=True),
            "level_c_host_cones": lambda: ipm.HipSystemBackend(P, A, cones, host_cones=True),
            "level_c_batched": lambda: ipm.HipSystemBackend(P, A, cones, batch_affine=True)}[name]()


@pytest.mark.parametrize("backend", DEVICE_SCALED)
def test_basic_genpow_on_the_device(backend):
    P, q, A, b, cones, exp = F.basic_genpow()
    be = _backend(backend, P, A, cones)
    r = ipm.solve(P, q, A, b, cones, be)
    r_cpu = ipm.solve(P, q, A, b, cones, G.ExpandedScipyBackend(P, A, cones))
    print(backend, r.status, r.iterations, r.obj_val, "cpu", r_cpu.iterations, r_cpu.obj_val)
    assert r.status == exp["status"] == ipm.SOLVED
    assert abs(r.obj_val - exp["obj"]) <= F.ATOL
    assert abs(r.obj_val - r_cpu.obj_val) <= F.ATOL
    assert be.ks.fallbacks == (0, 0)


def test_the_host_cone_route_refuses_a_generalized_power_cone():
    """level_c_host_cones hands the caller's (Hs, u, v, eta^2) over: there is no slot for p, q, r, and the entry point
    must say so instead of assembling a wrong K."""
    P, q, A, b, cones, exp = F.basic_genpow()
    be = _backend("level_c_host_cones", P, A, cones)
    with pytest.raises(_lib.HipKKTError, match="generalized power"):
        ipm.solve(P, q, A, b, cones, be)


_CPU = {}


def _cpu_run():
    if "r" not in _CPU:
        pb = problems.generalized_power_mix(copies=1)
        _CPU["pb"] = pb
        _CPU["r"] = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, G.ExpandedScipyBackend(pb.P, pb.A, pb.cones))
    return _CPU["pb"], _CPU["r"]


@pytest.mark.parametrize("backend", DEVICE_SCALED)
def test_generator_problem_on_the_device_against_cpu(backend):
    pb, r_cpu = _cpu_run()
    be = _backend(backend, pb.P, pb.A, pb.cones)
    r = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, be)
    print(backend, r.status, r.iterations, r.obj_val, "cpu", r_cpu.status, r_cpu.iterations, r_cpu.obj_val)
    assert r.status == ipm.SOLVED and r_cpu.status == ipm.SOLVED
    assert abs(r.obj_val - r_cpu.obj_val) <= F.ATOL
    assert be.ks.fallbacks == (0, 0)
