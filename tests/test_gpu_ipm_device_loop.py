"""`ipm_device.solve_device` -- the interior-point loop with the iterate resident in HBM, every cone operation between
the solves on the device -- on the reference's known answers and against `ipm.solve` over the same level-C backend with
host cone operations.  Iteration counts of both loops are printed (expected equal; alpha differs in the last bits, so
not asserted)."""
import numpy as np
import pytest

from cuclarabel_amd import ipm, problems
from cuclarabel_amd.cones import NonnegativeConeT, ExponentialConeT
from cuclarabel_amd.ipm_device import solve_device
from tests.golden.reference_fixtures import ALL

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the reference's own atol for its known answers (linear_solvers.jl: tol)


def _check(res, exp):
    assert res.status == exp["status"], (res.status, res.history[-1])
    if "x" in exp:
        assert np.linalg.norm(res.x - exp["x"]) < TOL
    if "obj" in exp:
        assert abs(res.obj_val - exp["obj"]) < TOL
        assert abs(res.obj_val_dual - exp["obj"]) < TOL


@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_known_answers_with_device_resident_iterate(name):
    P, q, A, b, cones, exp = ALL[name]()
    res = solve_device(P, q, A, b, cones)
    _check(res, exp)
    assert res.iterations < 30


def _both(pb):
    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones)
    ref = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, ipm.HipSystemBackend(pb.P, pb.A, pb.cones))
    print(f"\niterations: device loop {res.iterations}, host-vector loop {ref.iterations}; status {res.status} / {ref.status}")
    return res, ref


@pytest.mark.parametrize("maker", ["problems.small_mixed()", "problems.config2(n=3000)"])
def test_same_answer_as_the_host_vector_loop(maker):
    """the same status as ipm.solve + HipSystemBackend and a solution within 1e-7 relative (the reference's
    update-vs-fresh tolerance, data_updating.jl:28); config2(n=3000) has sparse second-order cones of dim 100"""
    res, ref = _both(eval(maker))
    assert res.status == ref.status
    for a, b in ((res.x, ref.x), (res.z, ref.z), (res.s, ref.s)):
        assert np.linalg.norm(a - b) <= 1e-7 * max(1.0, np.linalg.norm(b))
    assert abs(res.obj_val - ref.obj_val) <= 1e-7 * max(1.0, abs(ref.obj_val))


def test_iterate_stays_on_the_device_and_no_fallback_is_taken():
    pb = problems.small_mixed()
    seen = {}

    def inspect(tensors, backend):
        for name, t in tensors.items():
            assert t.is_cuda and t.dtype.is_floating_point, f"{name} is not a device tensor"
        seen.setdefault("backend", backend)
        seen.setdefault("fallbacks0", backend.ks.fallbacks)
        seen["calls"] = seen.get("calls", 0) + 1

    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspect)
    assert seen["calls"] == len(res.history) >= 2
    assert isinstance(res.x, np.ndarray) and isinstance(res.s, np.ndarray)
    assert seen["backend"].ks.fallbacks == seen["fallbacks0"] == (0, 0)


def test_nonsymmetric_cone_list_is_refused():
    import scipy.sparse as sp
    with pytest.raises(ValueError):
        solve_device(sp.identity(4, format="csc"), np.zeros(4), sp.identity(4, format="csc"), np.ones(4),
                     [NonnegativeConeT(1), ExponentialConeT()])
