"""`ipm_device.solve_device_batch_isolated`: a batch in which a member that fails ends alone.  Fixtures with known answers
(tests/golden/reference_fixtures, at the reference's own TOL = 1e-3, as tests/test_gpu_batch_ipm.py):

  unpoisoned       every member ends with its known answer and status, with and without the member refinement rule;
  poisoned update  the inspect hook sets z[0] of one member's second-order cone to -1 behind the residuals of iteration 2
                   (z0 < 0 puts z outside the cone whatever the rest: either z0^2 - ||z1||^2 <= 0, or z lies in -K and
                   w0^2 - ||w1||^2 = 2 + 2 <s, z> / (sscale zscale) <= 0), so that the kkt_update! of iteration 3 fails: that
                   member ends with NUMERICAL_ERROR at iteration 3, every other member still reaches its known answer and
                   SOLVED in as many iterations as without the poison or more than 3 -- with solve_device_batch every
                   member ends with NUMERICAL_ERROR at iteration 3;
  poisoned solve   (member refinement) the hook fills one member's rows of rx with NaN instead: the same expectations;
  non-finite data  a member with a NaN in q is refused with ValueError naming it.
"""
import numpy as np
import pytest

from cuclarabel_amd.ipm_device import solve_device_batch_isolated
from tests.golden.reference_fixtures import ALL

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the reference's own atol for its known answers (linear_solvers.jl: tol)
VICTIM = "basic_socp"                                        # nonnegative cone of 6, second-order cone of 3: z rows 6 .. 8
OTHERS = ("basic_qp", "basic_sdp", "basic_lp", "eq_constrained_1", "basic_qp_univariate")
POISON_AT = 2       # the hook's call behind the residuals of iteration 2: the update and the solves of iteration 3 read it
_CLEAN = {}


def batch(position):
    names = [VICTIM] + list(OTHERS) if position == "first" else list(OTHERS) + [VICTIM]
    return names, [ALL[k]() for k in names]


def clean(position, member_refinement):
    """the unpoisoned batch, solved once per (order, rule) and shared (never modified)"""
    key = (position, member_refinement)
    if key not in _CLEAN:
        names, parts = batch(position)
        _CLEAN[key] = solve_device_batch_isolated([pt[:5] for pt in parts], member_refinement=member_refinement)
    return _CLEAN[key]


def check_known(name, part, res):
    P, q, A, b, cones, exp = part
    assert res.status == exp["status"], (name, res.status, res.history[-1])
    if "x" in exp:
        assert np.linalg.norm(res.x - exp["x"]) < TOL, name
    if "obj" in exp:
        assert abs(res.obj_val - exp["obj"]) < TOL and abs(res.obj_val_dual - exp["obj"]) < TOL, name


@pytest.mark.parametrize("member_refinement", (True, False))
def test_unpoisoned_every_member_ends_with_its_known_answer(member_refinement):
    names, parts = batch("first")
    results = clean("first", member_refinement)
    print("\niterations per member:", {k: r.iterations for k, r in zip(names, results)})
    for name, part, res in zip(names, parts, results):
        check_known(name, part, res)
        assert res.iterations < 30 and len(res.history) == res.iterations + 1, name
    assert results[0].iterations > POISON_AT + 1, "the victim is still running when the poison comes"


def run_poisoned(position, member_refinement, what):
    names, parts = batch(position)
    v = names.index(VICTIM)
    x_off = np.concatenate([[0], np.cumsum([pt[0].shape[0] for pt in parts])])
    z_off = np.concatenate([[0], np.cumsum([pt[2].shape[0] for pt in parts])])
    calls = []

    def hook(tensors, backend):
        if len(calls) == POISON_AT:
            if what == "update":
                tensors["z"][int(z_off[v]) + 6] = -1.0
            else:
                tensors["rx"][int(x_off[v]):int(x_off[v + 1])] = float("nan")
        calls.append(1)

    results = solve_device_batch_isolated([pt[:5] for pt in parts], inspect=hook, member_refinement=member_refinement)
    base = clean(position, member_refinement)
    print(f"\n{what} poisoned, victim {position}, member rule {member_refinement}: statuses {[r.status for r in results]}, "
          f"iterations {[r.iterations for r in results]} (unpoisoned {[r.iterations for r in base]})")
    assert results[v].status == "NUMERICAL_ERROR" and results[v].iterations == POISON_AT + 1
    assert len(results[v].history) == POISON_AT + 1
    for k, (name, part, res) in enumerate(zip(names, parts, results)):
        if k == v:
            continue
        assert res.status == "SOLVED", (name, res.status)
        check_known(name, part, res)
        assert res.iterations >= min(base[k].iterations, POISON_AT + 2), (name, "the loop did not stop early")
        assert len(res.history) == res.iterations + 1
    assert len(calls) == max(len(r.history) for r in results)


@pytest.mark.parametrize("position", ("first", "last"))
@pytest.mark.parametrize("member_refinement", (True, False))
def test_a_poisoned_update_ends_its_member_alone(member_refinement, position):
    run_poisoned(position, member_refinement, "update")


@pytest.mark.parametrize("position", ("first", "last"))
def test_a_poisoned_solve_ends_its_member_alone(position):
    run_poisoned(position, True, "solve")


def test_a_member_with_non_finite_data_is_refused_by_name():
    names, parts = batch("first")
    probs = [list(pt[:5]) for pt in parts]
    q = np.array(probs[2][1], float)
    q[0] = np.nan
    probs[2][1] = q
    with pytest.raises(ValueError, match=r"member 2 .*non-finite.* q"):
        solve_device_batch_isolated([tuple(pb) for pb in probs])
