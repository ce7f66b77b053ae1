"""The preconditions of tests/test_gpu_member_refinement.py, asserted on the CPU: the stacks of
tests/member_refinement_cases.py are built in numpy, their K comes from the C oracle, and residual_reference.refine_loop
runs once per member on the member's block and once on the whole stack (the joint rule).

  - Every decision whose outcome a GPU test asserts is clear of its threshold by a factor >= 4 (refine_loop's margin).  For
    the stagnating member only the STOP decision is asserted: its ratio is about 1 -- >= 4 away from stop_ratio = 5, not
    from the accept threshold 1 --, so neither its accept decision nor its x is ever compared.
  - In the stagnating stack the joint rule is predicted to leave a healthy member with ||e_b|| >= 4 x the tolerance,
    where the member's own loop ends <= tolerance / 4: the gap the feature exists for.
  - In the stack of members scaled alike every member takes the joint loop's decisions (same rounds, every candidate
    accepted), which is what makes x bit-identical with the rule switched on and off.
  - In the reltol stack the small member needs its own ||b_b||: with the stack's ||b|| it would stop a round earlier.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import member_refinement_cases as mc
from tests import residual_reference as rr

STACKS = {"stagnating": mc.stagnating, "alike": mc.alike, "edges4": lambda: mc.edges(4), "edges5": lambda: mc.edges(5),
          "many700": mc.many, "relative": mc.relative}
_S = {}


def case(name):
    if name not in _S:
        st = STACKS[name]()
        K, dsigns = mc.oracle_image(st)
        rows, N = mc.member_rows(st)
        assert N == K.shape[0], "the members' rows cover the image"
        assert sorted(np.concatenate(rows).tolist()) == list(range(N))
        b = mc.rhs(st, N, rows)
        _S[name] = (st, K, dsigns, rows, b, mc.predict(st, K, dsigns, b, rows))
    return _S[name]


def test_the_image_is_block_diagonal_over_the_members_rows():
    """what member_rows claims: no entry of K couples two members -- the expansion rows of a sparse second-order cone
    included"""
    for name in STACKS:
        st, K, _, rows, _, _ = case(name)
        owner = np.empty(K.shape[0], dtype=np.int64)
        for k, r in enumerate(rows):
            owner[r] = k
        C = sp.coo_matrix(K)
        assert np.array_equal(owner[C.row], owner[C.col]), name


@pytest.mark.parametrize("name", list(STACKS))
def test_every_asserted_decision_is_clear_of_its_threshold(name):
    st, K, dsigns, rows, b, P = case(name)
    mc.assert_margins(st, P)
    for k, p in enumerate(P["members"]):
        if st.kinds[k] == "zero":
            assert p["rounds"] == 0 and not np.any(p["x"]), (name, k)
    print(f"\n[member refinement, host] {name}: rounds {[p['rounds'] for p in P['members']][:12]} joint {P['joint']['rounds']}")


def test_the_stagnating_stack_shows_the_gap():
    st, K, dsigns, rows, b, P = case("stagnating")
    assert [p["rounds"] for p in P["members"]] == [1, 2, 1, 0, 0]
    assert [p["stop"] for p in P["members"]] == ["ratio", "tol", "tol", "tol", "tol"]
    joint = P["joint"]
    assert joint["rounds"] == 1 and joint["stop"] == "ratio"
    assert rr.margin(joint["norms"][0] / joint["norms"][1], mc.STOP_RATIO) >= mc.MARGIN      # the joint STOP decision is clear too
    left = P["joint_member_norme"][1]
    assert left >= mc.MARGIN * st.abstol, ("the joint rule leaves the healthy scale-1 member above the tolerance", left)
    for k in (1, 2, 3, 4):
        assert P["members"][k]["norme"] <= st.abstol / mc.MARGIN, (k, P["members"][k]["norme"])


def test_members_scaled_alike_take_the_joint_decisions():
    st, K, dsigns, rows, b, P = case("alike")
    joint = P["joint"]
    assert joint["stop"] == "tol" and joint["margin"] >= mc.MARGIN and joint["rounds"] >= 2
    for p in P["members"]:
        # (every candidate accepted by the ratio rule, in the member's loop and in the joint one, until the tolerance ends both)
        assert p["rounds"] == joint["rounds"] and p["stop"] == "tol" and p["accepted_last"]
    # ... and no member is done a round early: its norm before the last round is still above the tolerance
    for p in P["members"]:
        assert p["norms"][-2] >= mc.MARGIN * st.abstol


def test_the_reltol_stack_is_decided_by_the_members_own_normb():
    st, K, dsigns, rows, b, P = case("relative")
    assert st.abstol == 0.0 and st.reltol > 0.0
    nbs = [p["normb"] for p in P["members"]]
    assert max(nbs) / min(nbs) >= 500.0
    small = int(np.argmin(nbs))
    p = P["members"][small]
    assert p["rounds"] == 2
    # the same member under the stack's ||b||: one round fewer, by a clear margin
    r = rows[small]
    Kb = sp.csr_matrix(K[r][:, r])
    other = rr.refine_loop(Kb, rr.HostFactor(Kb, dsigns[r], rr.REG_EPS), b[r], st.reltol * max(nbs), 0.0, mc.STOP_RATIO, mc.MAX_ITER)
    assert other["rounds"] == p["rounds"] - 1 and other["margin"] >= mc.MARGIN


def test_a_member_with_an_inf_leaves_the_other_predictions_alone():
    st, K, dsigns, rows, b, P = case("edges5")
    b2 = b.copy()
    b2[rows[3][0]] = np.inf
    Q = mc.predict(st, K, dsigns, b2, rows)
    assert Q["members"][3]["stop"] == "bad" and "joint" not in Q
    for k in (0, 1, 2, 4):
        assert Q["members"][k]["rounds"] == P["members"][k]["rounds"]


@pytest.mark.parametrize("name", ["edges64", "edges8"])
def test_the_single_member_cases_need_two_rounds(name):
    """nb = 1 (the GPU test compares bits with the joint path): the builder's problems of residual_reference, one with
    64 lanes per row and no long row, one with 8 lanes and four long rows."""
    c = rr.refinement_case(name, 1)
    K = rr.expected_image(c["P"], c["A"], c["hs"])
    f = rr.check_shape(K, c["spec"]["want"])
    assert (f["nlong"] > 0) == (name == "edges8")
    n, m = c["P"].shape[0], c["A"].shape[0]
    p = rr.refine_loop(K, rr.HostFactor(K, np.concatenate([np.ones(n), -np.ones(m)]), rr.REG_EPS), c["B"][:, 0], c["abstol"], 0.0,
                       mc.STOP_RATIO, mc.MAX_ITER)
    assert p["rounds"] == 2 and p["stop"] == "tol" and p["margin"] >= mc.MARGIN, (p["rounds"], p["norms"], p["margin"])
