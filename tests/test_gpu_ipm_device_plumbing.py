"""`solve_device(..., plumbing="device")`: the interior-point loop whose residuals, termination scalars, combined
right-hand side and step update are the library's own hipkkt_kkt_system_residuals / _combined_rhs / _add_step instead of
torch expressions over a second copy of P and A -- on the reference's known answers, against plumbing="torch", and with
`ipm_device._Csr` made to raise."""
import numpy as np
import pytest

from cuclarabel_amd import ipm_device, problems
from cuclarabel_amd.ipm_device import solve_device
from tests.golden.reference_fixtures import ALL

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the reference's own atol for its known answers (linear_solvers.jl: tol)


@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_known_answers_with_device_plumbing(name):
    P, q, A, b, cones, exp = ALL[name]()
    res = solve_device(P, q, A, b, cones, plumbing="device")
    assert res.status == exp["status"], (res.status, res.history[-1])
    if "x" in exp:
        assert np.linalg.norm(res.x - exp["x"]) < TOL
    if "obj" in exp:
        assert abs(res.obj_val - exp["obj"]) < TOL
        assert abs(res.obj_val_dual - exp["obj"]) < TOL
    assert res.iterations < 30


@pytest.mark.parametrize("maker", ["problems.small_mixed()", "problems.config2(n=3000)"])
def test_same_answer_as_the_torch_plumbing(maker):
    """the same status and a solution within 1e-7 relative (data_updating.jl:28); iteration counts printed, not asserted"""
    pb = eval(maker)
    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device")
    ref = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="torch")
    print(f"\niterations: device plumbing {res.iterations}, torch plumbing {ref.iterations}; status {res.status} / {ref.status}")
    assert res.status == ref.status
    for a, b in ((res.x, ref.x), (res.z, ref.z), (res.s, ref.s)):
        assert np.linalg.norm(a - b) <= 1e-7 * max(1.0, np.linalg.norm(b))
    assert abs(res.obj_val - ref.obj_val) <= 1e-7 * max(1.0, abs(ref.obj_val))


def test_device_plumbing_never_builds_a_torch_matrix(monkeypatch):
    class Raises:
        def __init__(self, *a, **k):
            raise AssertionError("plumbing='device' constructed ipm_device._Csr")

    monkeypatch.setattr(ipm_device, "_Csr", Raises)
    pb = problems.small_mixed()
    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device")
    assert res.status == "SOLVED", res.status
    with pytest.raises(AssertionError):
        solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="torch")
    with pytest.raises(ValueError):
        solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="numpy")


def test_iterate_stays_on_the_device_with_the_same_inspect_keys():
    pb = problems.small_mixed()
    seen, keys = {}, {}

    def inspector(tag):
        def inspect(tensors, backend):
            for name, t in tensors.items():
                assert t.is_cuda and t.dtype.is_floating_point, f"{name} is not a device tensor"
            keys.setdefault(tag, set(tensors))
            assert set(tensors) == keys[tag]
            seen.setdefault(tag + "backend", backend)
            seen.setdefault(tag + "fallbacks0", backend.ks.fallbacks)
            seen[tag + "calls"] = seen.get(tag + "calls", 0) + 1
        return inspect

    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspector("d"), plumbing="device")
    ref = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspector("t"), plumbing="torch")
    assert keys["d"] == keys["t"] and {"x", "s", "z", "rx", "rz", "rx_inf", "rz_inf", "Px", "q", "b"} <= keys["d"]
    assert seen["dcalls"] == len(res.history) >= 2 and seen["tcalls"] == len(ref.history)
    assert isinstance(res.x, np.ndarray) and isinstance(res.s, np.ndarray)
    assert seen["dbackend"].ks.fallbacks == seen["dfallbacks0"] == (0, 0)
