"""`ipm_device.solve_device_batch_refined`: the batch loop with the refinement's accept / stop rule applied per member
(hipkkt_kkt_system_set_member_refinement).  Every member ends with ITS answer, as under solve_device_batch -- and a
singular member in the stack no longer decides how far the others' solves are refined."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import problems
from cuclarabel_amd.cones import ZeroConeT
from cuclarabel_amd.ipm_device import solve_device, solve_device_batch, solve_device_batch_refined
from tests.golden.reference_fixtures import ALL

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the reference's own atol for its known answers (linear_solvers.jl: tol)


def test_every_fixture_ends_with_its_own_known_answer():
    """all 21 fixtures -- feasible, primal-infeasible and dual-infeasible members -- in ONE batch"""
    names = sorted(ALL)
    parts = [ALL[k]() for k in names]
    results = solve_device_batch_refined([pt[:5] for pt in parts])
    assert len(names) == 21
    print("\niterations per member:", {k: r.iterations for k, r in zip(names, results)})
    print("refinement rounds per member:", {k: r.kkt_ir_rounds for k, r in zip(names, results)})
    for name, (P, q, A, b, cones, exp), res in zip(names, parts, results):
        assert res.status == exp["status"], (name, res.status, res.history[-1])
        if "x" in exp:
            assert np.linalg.norm(res.x - exp["x"]) < TOL, name
        if "obj" in exp:
            assert abs(res.obj_val - exp["obj"]) < TOL and abs(res.obj_val_dual - exp["obj"]) < TOL, name
        assert res.iterations < 30 and len(res.history) == res.iterations + 1, name
        assert res.x.shape == (P.shape[0],) and res.z.shape == res.s.shape == (A.shape[0],)
    # every member's own total (a member that has ended stops counting: its right-hand sides are zero from then on)
    assert all(isinstance(r.kkt_ir_rounds, int) and r.kkt_ir_rounds >= 0 for r in results)


def _close(a, b):
    return np.linalg.norm(a - b) <= 1e-7 * max(1.0, np.linalg.norm(b))


def _singular_member(seed=77):
    """more equality rows than variables (K_b singular), consistent: 3 variables, 5 equality rows"""
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(rng.standard_normal((5, 3)))
    x0 = rng.standard_normal(3)
    return sp.identity(3, format="csc"), rng.standard_normal(3), A, A @ x0, [ZeroConeT(5)]


def test_healthy_members_beside_a_singular_one_end_as_they_do_alone():
    """the eight small_mixed members of tests/test_gpu_batch_ipm.py plus one singular member: every healthy member ends with
    its stand-alone status, and x, z, s within 1e-7 relative of solve_device(plumbing="device") (the project's tolerance for
    one answer by two routes).  The iteration counts are printed next to what solve_device_batch gives for the same batch;
    that second run is informative only."""
    run = lambda pb: solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device")
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
    batch = [(pb.P, pb.q, pb.A, pb.b, pb.cones) for pb in pbs] + [_singular_member()]
    results = solve_device_batch_refined(batch)
    joint = solve_device_batch(batch)
    print(f"\niterations: member rule {[r.iterations for r in results]}, joint rule {[r.iterations for r in joint]}, "
          f"alone {[r.iterations for r in alone]}")
    print(f"statuses: member rule {[r.status for r in results]}, joint rule {[r.status for r in joint]}")
    print(f"refinement rounds per member (member rule): {[r.kkt_ir_rounds for r in results]}; stack total (joint rule): "
          f"{joint[0].kkt_ir_rounds}")
    for pb, res, ref in zip(pbs, results, alone):
        assert res.status == ref.status, pb.name
        assert _close(res.x, ref.x) and _close(res.z, ref.z) and _close(res.s, ref.s), pb.name
