"""`ipm_device.solve_device_batch`: a batch of independent problems on one block-diagonal handle, every member with its own
tau, kappa, mu, step length, termination test and status.  tests/test_batch_joint_loop_host.py pins what the joint loop
does with such a stack (one infeasible member takes all of it along); here every member ends with ITS answer."""
import numpy as np
import pytest

from cuclarabel_amd import problems
from cuclarabel_amd.ipm_device import solve_device, solve_device_batch
from tests.golden.reference_fixtures import ALL

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the reference's own atol for its known answers (linear_solvers.jl: tol)
_KNOWN = {}


def _known(order):
    """the batch of all 21 fixtures, solved once per member order and shared (never modified)"""
    if order not in _KNOWN:
        names = sorted(ALL, reverse=(order == "reversed"))
        parts = [ALL[k]() for k in names]
        _KNOWN[order] = (names, parts, solve_device_batch([pt[:5] for pt in parts]))
    return _KNOWN[order]


def test_every_fixture_ends_with_its_own_known_answer():
    """all 21 fixtures -- feasible, primal-infeasible and dual-infeasible members -- in ONE batch"""
    names, parts, results = _known("sorted")
    assert len(names) == 21
    want = [pt[5]["status"] for pt in parts]
    assert want.count("SOLVED") >= 11 and want.count("PRIMAL_INFEASIBLE") >= 4 and want.count("DUAL_INFEASIBLE") >= 5
    print("\niterations per member:", {k: r.iterations for k, r in zip(names, results)})
    for name, (P, q, A, b, cones, exp), res in zip(names, parts, results):
        assert res.status == exp["status"], (name, res.status, res.history[-1])
        if "x" in exp:
            assert np.linalg.norm(res.x - exp["x"]) < TOL, name
        if "obj" in exp:
            assert abs(res.obj_val - exp["obj"]) < TOL and abs(res.obj_val_dual - exp["obj"]) < TOL, name
        assert res.iterations < 30 and len(res.history) == res.iterations + 1, name
        assert res.x.shape == (P.shape[0],) and res.z.shape == res.s.shape == (A.shape[0],)


def test_member_order_does_not_change_the_statuses():
    names, _, results = _known("sorted")
    rnames, _, rresults = _known("reversed")
    assert rnames == names[::-1]
    assert {k: r.status for k, r in zip(names, results)} == {k: r.status for k, r in zip(rnames, rresults)}


def _close(a, b):
    return np.linalg.norm(a - b) <= 1e-7 * max(1.0, np.linalg.norm(b))


@pytest.mark.parametrize("which", ("small_mixed", "config4"))
def test_every_member_as_its_own_stand_alone_solve(which):
    """all-QP batches, so that the start's LP / QP branch is the members' own: the same status, and x, z, s and the objective
    within 1e-7 relative (the project's tolerance for one answer by two routes, data_updating.jl:28).

    This is the test that a finished member must not disturb the others: seed 27 (11 iterations alone) runs on beside members
    that end after 9 and 10, and with their blocks left at the iterates they ended on it ended ALMOST_SOLVED after 15."""
    run = lambda pb: solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device")
    if which == "small_mixed":
        # eight seeds whose stand-alone solve converges: a member that ends ALMOST_SOLVED by itself (seed 25 does, on
        # insufficient progress) has no answer to compare at 1e-7
        pbs, alone = [], []
        for seed in range(21, 40):
            pb = problems.small_mixed(seed=seed)
            ref = run(pb)
            if ref.status == "SOLVED":
                pbs.append(pb)
                alone.append(ref)
            if len(pbs) == 8:
                break
        assert len(pbs) == 8
    else:
        pbs = [problems.config4(j, n=300) for j in range(4)]
        alone = [run(pb) for pb in pbs]
    results = solve_device_batch([(pb.P, pb.q, pb.A, pb.b, pb.cones) for pb in pbs])
    print(f"\n{which}: iterations in the batch {[r.iterations for r in results]}, alone {[r.iterations for r in alone]}")
    for pb, res, ref in zip(pbs, results, alone):
        assert res.status == ref.status, pb.name
        assert _close(res.x, ref.x) and _close(res.z, ref.z) and _close(res.s, ref.s), pb.name
        assert abs(res.obj_val - ref.obj_val) <= 1e-7 * max(1.0, abs(ref.obj_val)), pb.name


def test_a_finished_member_is_frozen_at_the_iterate_it_ended_on():
    """an easy and a hard member: the easy one's history stops at its own last iteration, and its result is the iterate of
    that iteration -- solving it alone to the same iteration count gives the same x"""
    from cuclarabel_amd.ipm import IPMSettings
    P, q, A, b, cones, _ = ALL["basic_qp_univariate"]()
    easy = (P, q, A, b, cones)
    hard_pb = problems.small_mixed(seed=5)
    hard = (hard_pb.P, hard_pb.q, hard_pb.A, hard_pb.b, hard_pb.cones)
    r_easy, r_hard = solve_device_batch([easy, hard])
    print(f"\niterations: easy {r_easy.iterations}, hard {r_hard.iterations}")
    assert r_easy.status == r_hard.status == "SOLVED"
    assert r_easy.iterations < r_hard.iterations
    assert len(r_easy.history) == r_easy.iterations + 1 and len(r_hard.history) == r_hard.iterations + 1
    assert [h["iter"] for h in r_easy.history] == list(range(r_easy.iterations + 1))
    ref = solve_device(*easy, plumbing="device")
    assert ref.status == "SOLVED"
    capped = solve_device(*easy, settings=IPMSettings(max_iter=r_easy.iterations), plumbing="device")
    print(f"alone: {ref.iterations} iterations; capped at the batch's count: {capped.iterations}")
    assert capped.iterations <= r_easy.iterations
    assert _close(r_easy.x, capped.x)


def test_iterate_stays_on_the_device_and_no_fallback_is_taken():
    pbs = [problems.small_mixed(seed=s) for s in (31, 32, 33)]
    seen = {}

    def inspect(tensors, backend):
        for name, t in tensors.items():
            assert t.is_cuda and t.dtype.is_floating_point, f"{name} is not a device tensor"
        seen.setdefault("backend", backend)
        seen.setdefault("fallbacks0", backend.ks.fallbacks)
        seen["calls"] = seen.get("calls", 0) + 1

    results = solve_device_batch([(pb.P, pb.q, pb.A, pb.b, pb.cones) for pb in pbs], inspect=inspect)
    assert seen["calls"] == max(len(r.history) for r in results) >= 2
    assert all(isinstance(r.x, np.ndarray) and isinstance(r.s, np.ndarray) for r in results)
    assert seen["backend"].ks.fallbacks == seen["fallbacks0"] == (0, 0)
