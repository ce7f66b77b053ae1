"""solver_device.DeviceSolver: the resident solver that re-solves after data updates.

  - without equilibration its solve IS solve_device*(plumbing="device"), bit for bit;
  - with equilibration (the default) it meets the reference's known answers at the reference's own tolerance;
  - the ten cases of the reference's test/OptTests/data_updating.jl, each a re-solve after an update against a fresh solver
    on the new data, and its no-ops;
  - after update_data a re-solve equals, bit for bit, the solve of a fresh solver built from the new data with the SAME
    equilibration: nothing stale survives an update (x, z, s, status, iterations, every history row);
  - a pattern mismatch raises ValueError and leaves the solver usable."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import ipm, ipm_device, problems
from tests.golden import data_updating_fixtures as U
from tests.golden import nonsymmetric_fixtures as NF
from tests.golden.reference_fixtures import ALL

pytestmark = pytest.mark.gpu

TOL = 1e-3          # linear_solvers.jl: tol (as tests/test_ipm_fixtures.py)


def solver(*a, **kw):
    from cuclarabel_amd.solver_device import DeviceSolver
    return DeviceSolver(*a, **kw)


def assert_same_result(r1, r2, tag=""):
    assert r1.status == r2.status and r1.iterations == r2.iterations, (tag, r1.status, r2.status, r1.iterations, r2.iterations)
    assert len(r1.history) == len(r2.history), tag
    for i, (h1, h2) in enumerate(zip(r1.history, r2.history)):
        for k in h1:
            assert h1[k] == h2[k] or (h1[k] != h1[k] and h2[k] != h2[k]), (tag, "history row", i, k, h1[k], h2[k])
    for name in ("x", "z", "s"):
        a, b = getattr(r1, name), getattr(r2, name)
        assert a.tobytes() == b.tobytes(), (tag, name, float(np.abs(a - b).max()))


# ------------------------------------------------------------------------------------------------ the loop is the loop
def test_without_equilibration_it_is_solve_device_bit_for_bit():
    pb = problems.small_mixed()
    ref = ipm_device.solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device")
    s = solver(pb.P, pb.q, pb.A, pb.b, pb.cones, equilibrate=False)
    assert s.equilibration.c == 1.0 and (s.equilibration.d == 1.0).all() and (s.equilibration.e == 1.0).all()
    res = s.solve()
    assert ref.status == ipm.SOLVED
    assert_same_result(res, ref, "small_mixed")
    assert res.obj_val == ref.obj_val and res.obj_val_dual == ref.obj_val_dual
    assert_same_result(s.solve(), ref, "small_mixed, solved again")           # always from the default start


def test_without_equilibration_it_is_solve_device_nonsymmetric_bit_for_bit():
    P, q, A, b, cones, exp = NF.basic_exp()
    ref = ipm_device.solve_device_nonsymmetric(P, q, A, b, cones, plumbing="device")
    s = solver(P, q, A, b, cones, equilibrate=False)
    assert ref.status == ipm.SOLVED
    assert_same_result(s.solve(), ref, "basic_exp")
    assert_same_result(s.solve(), ref, "basic_exp, solved again")


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_known_answers_with_equilibration(name):
    P, q, A, b, cones, exp = ALL[name]()
    res = solver(P, q, A, b, cones).solve()
    assert res.status == exp["status"], (res.status, res.history[-1])
    if "x" in exp:
        assert np.linalg.norm(res.x - exp["x"]) < TOL
    if "obj" in exp:
        assert abs(res.obj_val - exp["obj"]) < TOL
        assert abs(res.obj_val_dual - exp["obj"]) < TOL


# ------------------------------------------------------------------------------------------------ data_updating.jl
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_reference_data_updating_case(name):
    which, update, new = U.CASES[name]
    P, q, A, b, cones = U.updating_test_data()
    s1 = solver(P, q, A, b, cones)
    first = s1.solve()
    assert first.status == ipm.SOLVED
    getattr(s1, "update_" + which)(update())
    r1 = s1.solve()
    data = dict(P=P, q=q, A=A, b=b)
    data[which] = new()
    r2 = solver(data["P"], data["q"], data["A"], data["b"], cones).solve()
    assert r1.status == r2.status == ipm.SOLVED
    assert np.linalg.norm(r1.x - r2.x) <= U.TOL, (name, r1.x, r2.x)
    assert abs(r1.obj_val - r2.obj_val) <= 1e-6 * max(1.0, abs(r2.obj_val)), "the objective is the new data's"


def test_reference_data_updating_noops():
    """data_updating.jl:265-284"""
    P, q, A, b, cones = U.updating_test_data()
    s = solver(P, q, A, b, cones)
    r0 = s.solve()
    for fn in (s.update_P, s.update_A, s.update_q, s.update_b):
        fn(None)
        fn(np.zeros(0))
    s.update_data(None, None, None, None)
    s.update_data()
    s.update_q((np.zeros(0, np.int64), np.zeros(0)))
    assert_same_result(s.solve(), r0, "after the no-ops")


def test_update_forms_agree_and_device_tensors_are_taken():
    """vector, (index, values) over every position, sparse matrix, and a device tensor leave the same solver"""
    import torch
    P, q, A, b, cones = U.updating_test_data()
    P2 = sp.triu(sp.csc_matrix(np.array([[5.0, 0.5], [0.5, 3.0]])), format="csc")
    out = []
    for form in ("vector", "indexed", "matrix", "tensor"):
        s = solver(P, q, A, b, cones)
        arg = {"vector": P2.data, "indexed": (np.array([2, 0, 1]), P2.data[[2, 0, 1]]), "matrix": P2 + sp.triu(P2, 1).T,
               "tensor": torch.from_numpy(P2.data.copy()).to(s._c.dev)}[form]
        s.update_P(arg)
        out.append(s.solve())
        assert np.array_equal(s.P.data, P2.data)
    for r in out[1:]:
        assert_same_result(r, out[0])


# ------------------------------------------------------------------------------------------------ nothing stale
def _new_data(pb, only_b):
    rng = np.random.default_rng(5)
    x0 = pb.x0 + 0.05 * rng.standard_normal(pb.n)
    if only_b:
        return pb.P, pb.q, pb.A, pb.A @ x0 + pb.s0
    P2, A2 = pb.P.copy(), pb.A.copy()
    P2.data = P2.data * 2.0
    A2.data = A2.data * rng.uniform(0.8, 1.25, A2.nnz)
    return P2, pb.q * 1.1 + 0.01 * rng.standard_normal(pb.n), A2, A2 @ x0 + pb.s0


@pytest.mark.parametrize("only_b", [False, True], ids=["all_four", "only_b"])
def test_resolve_after_update_equals_a_fresh_solver_with_the_same_equilibration(only_b):
    pb = problems.small_mixed()
    s1 = solver(pb.P, pb.q, pb.A, pb.b, pb.cones)
    assert s1.equilibration.c != 1.0 or not (s1.equilibration.d == 1.0).all()
    r0 = s1.solve()
    assert r0.status == ipm.SOLVED
    P2, q2, A2, b2 = _new_data(pb, only_b)
    if only_b:
        s1.update_data(b=b2)
    else:
        s1.update_data(P=P2, q=q2, A=A2, b=b2)
    r1 = s1.solve()
    s2 = solver(P2, q2, A2, b2, pb.cones, equilibration=s1.equilibration)
    r2 = s2.solve()
    assert r2.status == ipm.SOLVED
    assert_same_result(r1, r2, "re-solve against a fresh solver")
    assert r1.obj_val == r2.obj_val and r1.obj_val_dual == r2.obj_val_dual
    assert np.abs(r1.x - r0.x).max() > 1e-6, "the new data has another answer"


def test_pattern_mismatch_is_refused_and_the_solver_stays_usable():
    P, q, A, b, cones = U.updating_test_data()
    s = solver(P, q, A, b, cones)
    r0 = s.solve()
    with pytest.raises(ValueError, match="sparsity pattern"):
        s.update_P(sp.csc_matrix(np.array([[4.0, 0.0], [0.0, 2.0]])))              # an entry missing
    with pytest.raises(ValueError, match="sparsity pattern"):
        s.update_A(sp.csc_matrix(np.array([[-1.0, 1.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]])))      # an entry too many
    with pytest.raises(ValueError):
        s.update_q(np.ones(3))
    with pytest.raises(ValueError):
        s.update_b((np.array([0, 0]), np.array([1.0, 2.0])))                        # a repeated position
    with pytest.raises(ValueError):
        s.update_data(q=np.array([5.0, 5.0]), P=sp.identity(2, format="csc"))       # P is refused: q must not be applied either
    assert_same_result(s.solve(), r0, "after the refusals")
