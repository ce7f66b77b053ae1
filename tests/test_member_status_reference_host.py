"""The host model of tests/member_status_reference.py on the CPU, on the image the C oracle assembles:
  - fault-free, the model's eps_b equal the truth's (connected components of the image, no partition) bit for bit and the
    members' own regularised solves add up to the regularised solve of the whole stack;
  - every seeded fault (FAULTS) is caught by a case named here;
  - the case of the regularised-solve test has blocks with condition number below 1e3, and under the JOINT epsilon its
    solution lies at least 1e6 tolerances away: that assertion cannot pass without the members' own epsilons;
  - the status words are predicted where the poison was put, for every kind, member position and stack size."""
import numpy as np
import pytest

from tests import member_refinement_cases as mc
from tests import member_status_reference as ms

_IMG = {}


def image(make):
    st = make()
    if st.name not in _IMG:
        K, dsigns = ms.oracle_image(st)
        rows, N = ms.member_rows(st)
        assert N == K.shape[0]
        _IMG[st.name] = (st, K, dsigns, rows, mc.rhs(st, N, rows))
    return _IMG[st.name]


def solve_distance(K, dsigns, rows, eps, rhs, want):
    """per member: max |x_b - want_b| in units of the member's tolerance 100 cond 2^-52 max |want_b|"""
    x, cond = ms.member_solve(K, dsigns, rows, eps, rhs)
    return np.array([np.abs(x[r] - want[r]).max() / (ms.solve_tolerance(cond[b]) * np.abs(want[r]).max())
                     for b, r in enumerate(rows)]), cond


@pytest.mark.parametrize("make", ms.EPS_CASES, ids=lambda f: f.__name__)
def test_the_model_agrees_with_the_partition_free_truth(make):
    st, K, dsigns, rows, rhs = image(make)
    want, lab = ms.truth_eps(K)
    for b, r in enumerate(rows):
        assert np.all(lab[r] == b), "the members are the components of the image"
    eps = ms.member_eps(K.diagonal(), rows)
    assert np.array_equal(eps, want)
    assert eps.max() == ms.C0 + ms.C1 * np.abs(K.diagonal()).max(), "the largest eps_b is the joint epsilon"
    if st.nb > 1:
        assert eps.max() / eps.min() > 10.0, "the members' epsilons lie more than an order of magnitude apart"
    dist, _ = solve_distance(K, dsigns, rows, eps, rhs, ms.truth_solve(K, dsigns, rhs))
    assert dist.max() <= 1.0, dist.max()


def test_the_cases_cover_the_sizes_and_the_positions_of_the_maximum():
    st, K, dsigns, rows, _ = image(ms.case_sizes)
    assert [r.size for r in rows] == [1, 255, 256, 257, 10]
    d = np.abs(K.diagonal())
    arg = [int(np.flatnonzero(d[r] == d[r].max())[0]) for r in rows]
    assert arg[1] == rows[1].size - 1 and K.diagonal()[rows[1][-1]] < 0, "last row, a negative -Hs entry"
    assert arg[2] == 0, "first row"
    assert int(np.argmax(ms.member_eps(K.diagonal(), rows))) == 1, "the stack's maximum lies in another member than 2, 3, 4"
    top = rows[4][d[rows[4]] == d[rows[4]].max()]
    assert (top >= st.n + st.m).any(), "an expansion row holds member 4's maximum"
    st3, K3, _, rows3, _ = image(ms.case_three)
    d3 = np.abs(K3.diagonal())
    assert (rows3[0][d3[rows3[0]] == d3[rows3[0]].max()] >= st3.n + st3.m).any()
    stm, _, _, rowsm, _ = image(ms.case_many)
    assert stm.nb == 300 and image(ms.case_one)[0].nb == 1 and st3.nb == 3


CAUGHT_BY = {"joint_eps": ms.case_three, "neighbour_max": ms.case_sizes, "no_expansion_rows": ms.case_three}


@pytest.mark.parametrize("fault", sorted(CAUGHT_BY))
def test_every_seeded_fault_of_the_regulariser_is_caught(fault):
    st, K, dsigns, rows, rhs = image(CAUGHT_BY[fault])
    want_eps, _ = ms.truth_eps(K)
    frows, _ = ms.member_rows(st, fault)
    feps = ms.member_eps(K.diagonal(), frows, fault)
    x, cond = ms.member_solve(K, dsigns, frows, feps, rhs)
    want = ms.truth_solve(K, dsigns, rhs)
    n_m = st.n + st.m
    far = max(np.abs(x[r] - want[r]).max() / (ms.solve_tolerance(cond[b]) * np.abs(want[r[r < n_m]]).max())
              for b, r in enumerate(frows))
    assert not np.array_equal(feps, want_eps) or far > 1e6, (fault, far)
    assert far > 1e6, (fault, far)                        # (each of the three moves some member's solution as well)


def test_the_regularised_solve_case_separates_the_members_epsilon_from_the_joint_one():
    st, K, dsigns, rows, rhs = image(ms.case_three)
    eps = ms.member_eps(K.diagonal(), rows)
    want, cond = ms.member_solve(K, dsigns, rows, eps, rhs)
    assert cond.max() < 1e3, cond
    # smallest singular value of every regularised block >= |K_b| / cond: far from dynamic_regularization_eps = 1e-13
    for b, r in enumerate(rows):
        Kb = K[r][:, r].toarray() + np.diag(eps[b] * dsigns[r])
        assert np.linalg.svd(Kb, compute_uv=False).min() > 1e-3
    joint = ms.member_eps(K.diagonal(), rows, "joint_eps")
    dist, _ = solve_distance(K, dsigns, rows, joint, rhs, want)
    others = [b for b in range(st.nb) if eps[b] != joint[b]]
    assert len(others) == 2
    print("\ndistance of the joint-epsilon solution in tolerances:", dist, "cond:", cond)
    assert all(dist[b] >= 1e6 for b in others), dist


@pytest.mark.parametrize("nb", (3, 300))
def test_the_words_are_predicted_where_the_poison_was_put(nb):
    st, where = ms.attribution_stack(nb)
    for kind in ("soc", "nn", "psd"):
        for b in (0, nb // 2, nb - 1):
            s, z, poison = ms.poisoned(st, where, kind, b)
            assert np.flatnonzero((s != st.s) | (z != st.z)).size in (1, 3)
            W = ms.member_words(st, poison)
            want = np.zeros((nb, 2))
            want[b, 1 if kind == "nn" else 0] = 1.0       # (by construction: poisoned() wrote into member b's rows)
            assert np.array_equal(W, want), (kind, b)
            assert not np.array_equal(ms.member_words(st, poison, "next_member"), want), "the fault is caught"
    assert np.array_equal(ms.member_words(st, []), np.zeros((nb, 2)))
