"""The refinement rule per member (hipkkt_kkt_system_set_member_refinement; csrc/batch_kernels.hip: k_member_residual,
k_member_long_finish, k_member_ir_round; csrc/hipkkt.hip: kkt_solve_core_members) through level B kktsolver_setrhs /
kktsolver_solve on a partitioned handle, so that the right-hand side is free.

The stacks and the host prediction are those of tests/member_refinement_cases.py; tests/
test_member_refinement_reference_host.py asserts their margins on the CPU, and every case here asserts them again on the
image the device holds before it asks the device: every decision compared is clear of its threshold by a factor >= 4,
so that the round counts are a property of the problem, not of rounding.  Settings as residual_reference.refinement_case:
static regularisation 1e-4 constant with proportional part 0, reltol 0 except in the reltol case.

For every case: member b's rounds in member_refinement_info() equal the prediction, last_ir_iterations equals the largest
of them; where a member stops by tolerance its TRUE residual (residual_exact on its rows of the un-regularised K) is
<= abstol + max residual_bound -- derived, not measured: the device's own residual is within residual_bound of the true
one; a zero member's rows of x are exactly 0 with 0 rounds; ks.fallbacks stays (0, 0).

A member with a sparse second-order cone owns two expansion rows whose unknowns level B does not return.  They are taken
from the member's z rows by the expansion rows themselves (y_p = -K[p, z] z / K[p, p]); the device's y differs from that
by e_p / K[p, p] with |e_p| <= the tolerance, which moves row i of the residual by at most sum_p |K[i, p]| / |K[p, p]|
tolerances: the limit of such a member is (abstol + bound) (1 + max_i sum_p |K[i, p] / K[p, p]|).
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import member_refinement_cases as mc
from tests import residual_reference as rr

pytestmark = pytest.mark.gpu

_S = {}


def handle(st):
    """(ks, system, K, dsigns, rows) for a stack: factorised at (s, z), partitioned; once per session."""
    if st.name not in _S:
        from cuclarabel_amd import _lib
        from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
        ks = HipKKTSolver(st.P, st.A, st.cones, settings=_lib.default_settings(**st.settings()))
        assert ks.kktsolver_update_from_sz(st.s, st.z)
        assert ks.diagonal_regularizer == rr.REG_EPS
        system = HipKKTSystem(ks)
        system.init(np.zeros(st.n), np.zeros(st.m))
        system.set_problems(st.blocks)
        K = rr.sym_of(ks)
        rows, N = mc.member_rows(st)
        assert N == ks.N
        _S[st.name] = (ks, system, K, np.asarray(ks.maps()["dsigns"], np.float64), rows)
    return _S[st.name]


def solve(ks, st, b):
    ks.kktsolver_setrhs(b[:st.n], b[st.n:st.n + st.m])
    x, z = np.zeros(st.n), np.zeros(st.m)
    ok = ks.kktsolver_solve(x, z)
    return ok, np.concatenate([x, z]), ks.last_ir_iterations


def check_members(tag, st, K, rows, b, xz, info, P, skip=()):
    """rounds, the true residual where a member stops by tolerance, zero members."""
    n_m = st.n + st.m
    worst = (0.0, None)
    for k, p in enumerate(P["members"]):
        if k in skip:
            continue
        where = f"{tag} member {k} ({st.kinds[k]}) norms {['%.1e' % v for v in p['norms']]}"
        assert int(info[k, 0]) == p["rounds"], (where, info[k])
        assert info[k, 3] == 0.0, where
        r = rows[k]
        own = r[r < n_m]
        if st.kinds[k] == "zero":
            assert not np.any(xz[own]) and info[k, 1] == 0.0 and info[k, 2] == 0.0, where
            continue
        assert info[k, 2] == np.abs(b[r]).max(), (where, "||b_b||")
        if st.kinds[k] == "singular" or p["stop"] != "tol":
            continue
        tol = mc.member_tol(st, p)
        assert info[k, 1] <= tol, (where, info[k, 1], tol)
        Kb = sp.csr_matrix(K[r][:, r])
        xb = np.zeros(r.size)
        xb[r < n_m] = xz[own]
        factor = 1.0
        exp = np.flatnonzero(r >= n_m)
        if exp.size:                                     # the expansion unknowns from their own rows (see the head comment)
            D = Kb.diagonal()[exp]
            Kd = Kb.toarray()
            xb[exp] = -(Kd[exp][:, r < n_m] @ xz[own]) / D
            factor += np.abs(Kd[:, exp] / D).sum(axis=1)[r < n_m].max()
        hi, lo = rr.residual_exact(Kb, xb, b[r])
        true = np.abs(hi[r < n_m]).max()
        limit = (tol + rr.residual_bound(Kb, xb, b[r]).max()) * factor
        worst = max(worst, (true / limit, where))
        assert true <= limit, (where, true, limit)
    print(f"\n[member refinement] {tag}: rounds {[int(v) for v in info[:12, 0]]}; worst true residual / limit {worst[0]:.2e} ({worst[1]})")


def run_case(st, b=None, depth=None):
    ks, system, K, dsigns, rows = handle(st)
    b = mc.rhs(st, ks.N, rows) if b is None else b
    P = mc.predict(st, K, dsigns, b, rows)
    mc.assert_margins(st, P)
    system.set_member_refinement(True)
    if depth is not None:
        assert ks.speculative_rounds(depth) == depth
    ok, xz, last = solve(ks, st, b)
    info = system.member_refinement_info()
    assert ks.fallbacks == (0, 0)
    return ok, xz, last, info, P, b


# ------------------------------------------------------------------------------------------------ a. the stagnating stack
def test_a_stagnating_member_no_longer_ends_the_others_refinement():
    st = mc.stagnating()
    ks, system, K, dsigns, rows = handle(st)
    ok, xz, last, info, P, b = run_case(st)
    assert ok
    want = [p["rounds"] for p in P["members"]]
    assert want == [1, 2, 1, 0, 0]
    assert [int(v) for v in info[:, 0]] == want and last == max(want)
    check_members("stagnating", st, K, rows, b, xz, info, P)
    # every healthy member meets the tolerance, by its true residual
    for k in (1, 2, 3):
        r = rows[k]
        hi, _ = rr.residual_exact(sp.csr_matrix(K[r][:, r]), xz[r], b[r])
        assert np.abs(hi).max() <= st.abstol + rr.residual_bound(sp.csr_matrix(K[r][:, r]), xz[r], b[r]).max()
    # the same handle with the rule switched off: the joint loop stops after one round and leaves member 1 above it
    system.set_member_refinement(False)
    ok, xj, lastj = solve(ks, st, b)
    assert ok and lastj == P["joint"]["rounds"] == 1
    r = rows[1]
    hi, _ = rr.residual_exact(sp.csr_matrix(K[r][:, r]), xj[r], b[r])
    left = np.abs(hi).max()
    print(f"[member refinement] stagnating: member 1 under the joint rule {left:.2e}, predicted {P['joint_member_norme'][1]:.2e}, "
          f"tolerance {st.abstol:.1e}")
    assert P["joint_member_norme"][1] >= mc.MARGIN * st.abstol
    assert left > st.abstol, "the joint rule was predicted to leave this member at >= 4 x the tolerance"
    assert ks.fallbacks == (0, 0)


# ------------------------------------------------------------------------------------------------ b. nb = 1: the joint path's bits
@pytest.mark.parametrize("name", ["edges64", "edges8"], ids=["64-lanes-no-long-row", "8-lanes-long-rows"])
def test_b_one_member_is_bit_for_bit_the_joint_path(name):
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    case = rr.refinement_case(name, 1)
    ks = HipKKTSolver(case["P"], case["A"], case["cones"], settings=_lib.default_settings(**case["settings"]))
    assert ks.kktsolver_update(case["hs"])
    K = rr.sym_of(ks)
    f = rr.check_shape(K, case["spec"]["want"])
    assert (f["nlong"] > 0) == (name == "edges8")
    system = HipKKTSystem(ks)
    system.init(np.zeros(ks.n), np.zeros(ks.m))
    system.set_problems([(ks.n, ks.m)])
    b = case["B"][:, 0]
    got = []
    for on in (False, True, False, True):
        system.set_member_refinement(on)
        ks.kktsolver_setrhs(b[:ks.n], b[ks.n:])
        x, z = np.zeros(ks.n), np.zeros(ks.m)
        assert ks.kktsolver_solve(x, z)
        got.append((np.concatenate([x, z]), ks.last_ir_iterations))
        if on:
            info = system.member_refinement_info()
            assert info.shape == (1, 4) and int(info[0, 0]) == got[-1][1] and info[0, 3] == 0.0
            assert info[0, 2] == np.abs(b).max() and 0.0 < info[0, 1] <= case["abstol"]
    assert got[0][1] == 2, "the case needs two rounds (tests/test_member_refinement_reference_host.py)"
    for g in got[1:]:
        assert g[1] == got[0][1] and g[0].tobytes() == got[0][0].tobytes()
    assert ks.fallbacks == (0, 0)


# ------------------------------------------------------------------------------------------------ c. members that decide alike
def test_c_members_scaled_alike_give_the_joint_paths_bits():
    st = mc.alike()
    ks, system, K, dsigns, rows = handle(st)
    ok, xz, last, info, P, b = run_case(st)
    assert ok and last == P["joint"]["rounds"] and all(p["rounds"] == last for p in P["members"])
    check_members("alike", st, K, rows, b, xz, info, P)
    system.set_member_refinement(False)
    ok, xj, lastj = solve(ks, st, b)
    assert ok and lastj == last and xj.tobytes() == xz.tobytes()
    assert ks.fallbacks == (0, 0)


# ------------------------------------------------------------------------------------------------ d. the edge shapes
@pytest.mark.parametrize("nb", [4, 5])
def test_d_edge_shapes(nb):
    """a member of one x row; a member whose only z rows are a sparse second-order cone of dimension 5; members of 32 and of
    33 rows (a chunk of the 8-lane kernel, and one row more); nb = 5: a zero member behind them"""
    st = mc.edges(nb)
    ks, system, K, dsigns, rows = handle(st)
    assert rr.shape_facts(K)["lanes"] == 8 and [r.size for r in rows][:4] == [1, 10, 32, 33]
    assert (rows[1] >= st.n + st.m).sum() == 2, "two expansion rows"
    ok, xz, last, info, P, b = run_case(st)
    assert ok and last == max(p["rounds"] for p in P["members"])
    assert len({p["rounds"] for p in P["members"]}) >= 2
    check_members(st.name, st, K, rows, b, xz, info, P)


def test_d_seven_hundred_members_of_three_rows():
    st = mc.many(700)
    ks, system, K, dsigns, rows = handle(st)
    assert all(r.size == 3 for r in rows)
    ok, xz, last, info, P, b = run_case(st)
    assert ok and info.shape == (700, 4)
    want = np.array([p["rounds"] for p in P["members"]])
    assert sorted(set(want.tolist())) == [0, 1, 2]
    assert np.array_equal(info[:, 0].astype(int), want) and last == want.max()
    check_members(st.name, st, K, rows, b, xz, info, P)


# ------------------------------------------------------------------------------------------------ e. reltol, the member's own ||b_b||
def test_e_relative_tolerance_uses_the_members_own_normb():
    st = mc.relative()
    ks, system, K, dsigns, rows = handle(st)
    ok, xz, last, info, P, b = run_case(st)
    assert ok
    nbs = [p["normb"] for p in P["members"]]
    assert max(nbs) / min(nbs) >= 500.0
    small = int(np.argmin(nbs))
    assert P["members"][small]["rounds"] == 2 and int(info[small, 0]) == 2      # (one fewer under the stack's ||b||: host test)
    assert last == 2
    check_members(st.name, st, K, rows, b, xz, info, P)


# ------------------------------------------------------------------------------------------------ f. an Inf in one member
def test_f_an_inf_marks_its_member_alone():
    st = mc.edges(5)
    ks, system, K, dsigns, rows = handle(st)
    b = mc.rhs(st, ks.N, rows)
    b[rows[3][0]] = np.inf
    ok, xz, last, info, P, b = run_case(st, b=b)
    assert not ok, "the status of the solve stays joint: HIPKKT_NUMERIC_FAILURE"
    assert info[:, 3].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]
    assert int(info[3, 0]) == 0 and np.isinf(info[3, 1]) and np.isinf(info[3, 2])
    for k in (0, 1, 2, 4):
        assert int(info[k, 0]) == P["members"][k]["rounds"], (k, info[k])
        if P["members"][k]["stop"] == "tol" and st.kinds[k] != "zero":
            assert info[k, 1] <= st.abstol
    assert last == max(P["members"][k]["rounds"] for k in (0, 1, 2, 4))
    # the handle is as good as before: the finite right-hand side again
    ok, xz, last, info, P, b = run_case(st)
    assert ok and not np.any(info[:, 3])
    check_members("after-inf", st, K, rows, b, xz, info, P)


# ------------------------------------------------------------------------------------------------ g. speculation
@pytest.mark.parametrize("name", ["stagnating", "edges5"])
def test_g_speculation_does_not_change_the_result(name):
    st = mc.stagnating() if name == "stagnating" else mc.edges(5)
    ks, system, K, dsigns, rows = handle(st)
    got = []
    most = None
    for depth in (0, 2, 5):
        ok, xz, last, info, P, b = run_case(st, depth=depth)
        most = max(p["rounds"] for p in P["members"])
        assert ok and last == most == 2          # (depths: none, the exact count, more than it)
        got.append((xz, info))
    healthy = np.concatenate([rows[k][rows[k] < st.n + st.m] for k in range(st.nb) if st.kinds[k] != "singular"])
    for xz, info in got[1:]:
        assert np.array_equal(info[:, 0], got[0][1][:, 0])
        assert xz[healthy].tobytes() == got[0][0][healthy].tobytes()      # (the stagnating member's x is never compared)


# ------------------------------------------------------------------------------------------------ h. the switch
def test_h_needs_a_partition_and_goes_with_it():
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    st = mc.alike()
    ks = HipKKTSolver(st.P, st.A, st.cones, settings=_lib.default_settings(**st.settings()))
    assert ks.kktsolver_update_from_sz(st.s, st.z)
    system = HipKKTSystem(ks)
    system.init(np.zeros(st.n), np.zeros(st.m))
    rc = _lib.lib().hipkkt_kkt_system_set_member_refinement(ks._h, 1)
    assert rc == -1 and b"partition" in _lib.lib().hipkkt_last_error()          # HIPKKT_ERR_ARG
    with pytest.raises(_lib.HipKKTError, match="partition"):
        system.set_member_refinement(True)
    system.set_problems(st.blocks)
    with pytest.raises(_lib.HipKKTError, match="not enabled"):
        system.member_refinement_info()
    system.set_member_refinement(True)
    with pytest.raises(_lib.HipKKTError, match="no solve"):
        system.member_refinement_info()
    rows, N = mc.member_rows(st)
    b = mc.rhs(st, N, rows)
    ok, xz, last = solve(ks, st, b)
    assert ok and system.member_refinement_info().shape == (st.nb, 4)
    # replacing the partition switches the rule off; so does clearing it
    system.set_problems([(st.n, st.m)])
    with pytest.raises(_lib.HipKKTError, match="not enabled"):
        system.member_refinement_info()
    ok, x1, _ = solve(ks, st, b)
    assert ok
    system.set_member_refinement(True)
    system.set_problems(None)
    with pytest.raises(_lib.HipKKTError, match="not enabled"):
        system.member_refinement_info()
    ok, x2, _ = solve(ks, st, b)
    assert ok and x2.tobytes() == x1.tobytes()
    assert ks.fallbacks == (0, 0)
