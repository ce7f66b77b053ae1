"""solver_device.DeviceBatchSolver on a batch of eight `small_mixed` members (the generator and the seeds of
tests/test_gpu_batch_ipm.py), one member's q multiplied by 1e4 so that the members' cost scalings differ:

  - a re-solve after update_data / update_data_stack equals, bit for bit, a new solver built from the updated data with
    the same equilibrations;
  - every member against its own stand-alone DeviceSolver with that member's equilibration: the same status, the primal
    objectives within the sum of the two gap tolerances;
  - equilibrate=False is, bit for bit, solve_device_batch / _refined / _isolated on the same problems;
  - wrong argument forms of update_data raise ValueError before anything changes."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import problems
from cuclarabel_amd.ipm import IPMSettings

pytestmark = pytest.mark.gpu

BIG_Q = 5            # the member whose q is multiplied by 1e4


@pytest.fixture(scope="module")
def members():
    """eight seeds of small_mixed whose stand-alone solve converges, as tests/test_gpu_batch_ipm.py picks them"""
    from cuclarabel_amd.ipm_device import solve_device
    pbs = []
    for seed in range(21, 40):
        pb = problems.small_mixed(seed=seed)
        if solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device").status == "SOLVED":
            pbs.append(pb)
        if len(pbs) == 8:
            break
    assert len(pbs) == 8
    out = [(sp.triu(sp.csc_matrix(pb.P), format="csc"), np.array(pb.q, float), sp.csc_matrix(pb.A), np.array(pb.b, float),
            list(pb.cones)) for pb in pbs]
    P, q, A, b, cones = out[BIG_Q]
    out[BIG_Q] = (P, 1e4 * q, A, b, cones)
    return out


@pytest.fixture(scope="module")
def resident(members):
    """(the solver, its first results): shared, and left as built by the tests that only read it"""
    from cuclarabel_amd.solver_device import DeviceBatchSolver
    S = DeviceBatchSolver(members)
    return S, S.solve()


def same_value(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def assert_same_results(got, want, tag, objectives=True):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        where = f"{tag}: member {k}"
        assert g.status == w.status and g.iterations == w.iterations, (where, g.status, w.status, g.iterations, w.iterations)
        for name in ("x", "z", "s"):
            assert getattr(g, name).tobytes() == getattr(w, name).tobytes(), (where, name)
        assert len(g.history) == len(w.history), where
        for i, (hg, hw) in enumerate(zip(g.history, w.history)):
            assert hg.keys() == hw.keys() and all(same_value(hg[key], hw[key]) for key in hg), (where, "history row", i, hg, hw)
        assert g.kkt_ir_rounds == w.kkt_ir_rounds, where
        if objectives:
            assert same_value(float(g.obj_val), float(w.obj_val)) and same_value(float(g.obj_val_dual), float(w.obj_val_dual)), where


def test_the_members_cost_scalings_differ(resident):
    S, results = resident
    c = np.array([eq.c for eq in S.equilibrations])
    print(f"\nc_b = {c.tolist()}")
    assert c[BIG_Q] < np.delete(c, BIG_Q).min(), "the member with the large q has the smallest cost scaling"
    assert len(results) == 8 and all(r.x.shape == (m[0].shape[0],) for r, m in zip(results, S._c.members))


def test_resident_equals_fresh_bit_for_bit(members):
    import torch
    from cuclarabel_amd.solver_device import DeviceBatchSolver
    S = DeviceBatchSolver(members)
    first = S.solve()
    assert_same_results(S.solve(), first, "a second solve of the same data")
    rng = np.random.default_rng(7)
    new = [list(mb) for mb in members]
    # member 3: a new P (pattern kept), part of q by position, all of b
    P3 = new[3][0].copy()
    P3.sort_indices()
    f = rng.uniform(0.9, 1.1, P3.shape[0])                               # F P F: positive semidefinite like P
    P3.data = P3.data * (f[P3.indices] * f[np.repeat(np.arange(P3.shape[0]), np.diff(P3.indptr))])
    idx = np.array([new[3][1].size - 1, 0])
    q3 = new[3][1].copy()
    q3[idx] = q3[idx] * 1.5 + 0.25
    b3 = new[3][3] * rng.uniform(0.98, 1.02, new[3][3].size)
    S.update_data(3, P=P3, q=(idx, q3[idx]), b=b3)
    new[3][0], new[3][1], new[3][3] = P3, q3, b3
    # the whole stack: every member's q (a device tensor, by pointer) and b (numpy)
    for k in range(len(new)):
        new[k][1] = new[k][1] * rng.uniform(0.95, 1.05, new[k][1].size)
        new[k][3] = new[k][3] * (1.0 + 0.01 * (k % 3))
    q_stack = torch.from_numpy(np.concatenate([mb[1] for mb in new])).to(S._c.dev)
    S.update_data_stack(q=q_stack, b=np.concatenate([mb[3] for mb in new]))
    again = S.solve()
    fresh = DeviceBatchSolver([tuple(mb) for mb in new], equilibrations=S.equilibrations).solve()
    print(f"\nresident after the updates: {[(r.status, r.iterations) for r in again]}")
    assert_same_results(again, fresh, "resident against fresh")
    assert any(a.x.tobytes() != f.x.tobytes() for a, f in zip(again, first)), "the updates changed the answers"


def test_every_member_against_its_stand_alone_solver(members, resident):
    """the same status; where both are SOLVED the primal objectives agree within 2 (tol_gap_abs + tol_gap_rel max(|p_alone|,
    |p_batch|)): each is within its own gap tolerance of the optimum.  x is not compared."""
    from cuclarabel_amd.solver_device import DeviceSolver
    S, results = resident
    st = IPMSettings()
    alone = [DeviceSolver(*mb, equilibration=eq).solve() for mb, eq in zip(members, S.equilibrations)]
    print(f"\niterations in the batch {[r.iterations for r in results]}, alone {[r.iterations for r in alone]}")
    print(f"statuses in the batch {[r.status for r in results]}, alone {[r.status for r in alone]}")
    for k, (res, ref) in enumerate(zip(results, alone)):
        print(f"member {k}: objective in the batch {float(res.obj_val)!r}, alone {float(ref.obj_val)!r}")
    # (observed on an MI355X: 12, 11, 10, 10, 9, 15, 10, 10 iterations both ways)
    assert [r.iterations for r in results] == [r.iterations for r in alone]
    for k, (res, ref) in enumerate(zip(results, alone)):
        assert res.status == ref.status, k
        if res.status == "SOLVED":
            bound = 2 * (st.tol_gap_abs + st.tol_gap_rel * max(abs(ref.obj_val), abs(res.obj_val)))
            assert abs(res.obj_val - ref.obj_val) <= bound, (k, res.obj_val, ref.obj_val, bound)


@pytest.mark.parametrize("member_refinement,isolate", [(True, True), (True, False), (False, False)])
def test_without_equilibration_it_is_the_batch_loop_bit_for_bit(members, member_refinement, isolate):
    """scalings of one and c_b = 1: x, z, s, status, iteration count, refinement rounds and every history row of every
    member; the objectives (there from the host's data, here from the residual pass) are the last history row's costs"""
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.solver_device import DeviceBatchSolver
    if isolate:
        want = ipm_device.solve_device_batch_isolated(members, member_refinement=member_refinement)
    else:
        want = (ipm_device.solve_device_batch_refined if member_refinement else ipm_device.solve_device_batch)(members)
    S = DeviceBatchSolver(members, equilibrate=False, member_refinement=member_refinement, isolate=isolate)
    assert all(eq.c == 1.0 and (eq.d == 1.0).all() and (eq.e == 1.0).all() for eq in S.equilibrations)
    got = S.solve()
    assert_same_results(got, want, f"member_refinement={member_refinement}, isolate={isolate}", objectives=False)
    for g, w in zip(got, want):
        if g.status == "SOLVED":
            assert g.obj_val == w.history[-1]["pcost"] and g.obj_val_dual == w.history[-1]["dcost"]


def test_wrong_argument_forms_raise_before_anything_changes(members):
    from cuclarabel_amd.solver_device import DeviceBatchSolver
    S = DeviceBatchSolver(members)
    before = S.solve()
    P0, q0, A0, b0, _ = members[0]
    good_q = 2.0 * q0
    with pytest.raises(ValueError, match="member"):
        S.update_data(8, q=good_q)
    with pytest.raises(ValueError, match="member"):
        S.update_data(-1, q=good_q)
    other = sp.csc_matrix(A0).copy()
    other.data[0] = 0.0
    other.eliminate_zeros()                                              # one stored entry fewer
    with pytest.raises(ValueError, match="pattern"):
        S.update_data(0, q=good_q, A=other)                              # (q is fine: it must not be applied)
    with pytest.raises(ValueError, match="distinct"):
        S.update_data(0, b=2.0 * b0, q=(np.array([1, 1]), np.ones(2)))
    with pytest.raises(ValueError, match="distinct"):
        S.update_data(0, q=(np.array([q0.size]), np.ones(1)))          # a position of the next member
    with pytest.raises(ValueError, match="length"):
        S.update_data(0, P=2.0 * P0.data, b=np.ones(b0.size + 1))
    with pytest.raises(ValueError, match="length"):
        S.update_data_stack(q=np.ones(q0.size))                          # a member's vector is not the stack's
    with pytest.raises(ValueError, match="whole vectors"):
        S.update_data_stack(q=good_q.sum() * np.ones(1), P=P0)
    assert_same_results(S.solve(), before, "after the refused updates")
