"""The three refinement drivers (csrc/hipkkt.hip: kkt_solve_core with the accept / stop rule on the device in k_ir_round,
kkt_solve_multi_core, kkt_solve_multi_core_rm) on problems where refinement is NECESSARY by a wide margin, judged
without a measured tolerance.

Settings: static regularisation 1e-4 (constant; proportional part 0), so that the bare solve of the regularised factor
is wrong at the 1e-4 level and every round gains about four digits; reltol 0 and a purely absolute tolerance; columns
b_c = 10^(-3c) x random, so that the columns of one call need DIFFERENT numbers of rounds; one all-zero column; one
column whose first solve already meets the tolerance.  tests/residual_reference.py restates the reference's loop
(kktsolver_directldl.jl:389-449) in numpy over a host LU of the regularised K and predicts, per column, the residual
norms and the round count.  Every case asserts on the host, before the device is asked, that the first residual is at
least 1e4 x the tolerance and that EVERY accept / stop comparison of every column is clear of its threshold by a factor
of 4 or more -- so that the round counts are a property of the problem, not of rounding.

Per column: (a) rounds = the prediction = the C oracle's (where it runs the case); (b) the TRUE residual of the
returned x, by residual_exact on the un-regularised K, is <= abstol + max_i residual_bound wherever the loop stops by
tolerance (derived: the device's own residual is within residual_bound of the true one); (d) the zero column is exactly 0.

(c) of the plan -- a column stopped by the ratio rule -- cannot be reached under the 4 x margin rule: a ratio below
stop_ratio = 5 that is clear of 5 by 4 x is <= 1.25, and clear of 1 by 4 x then means <= 0.25: a candidate four times
WORSE than its predecessor, which refinement with a quasi-definite regularised factor (error map eps D (K + eps D)^-1,
norm < 1) does not produce.  The iterate comparison it asked for is made where the loop ends by the round cap.

Predicted norm sequences (column 0 | 1e-3 column | 1e-6 column | 1e-9 column), see residual_reference.REFINE_ABSTOL:
  edges64, abstol 3e-9:  2e-4 -> 3e-8 -> 5e-12 (2 rounds) | 3e-7 -> 4e-11 (1) | 4e-10 (0) | 2e-13 (0)
  edges8,  abstol 5e-9:  7e-4 -> 2e-7 -> 5e-11 (2 rounds) | 8e-7 -> 2e-10 (1) | 6e-10 (0) | 6e-13 (0)
  accept320k, abstol 1e-9:  5e-4 -> 7e-8 -> 9e-12 (2 rounds)
"""
import numpy as np
import pytest

from tests import residual_reference as rr
from tests.cone_reference import Worst

pytestmark = pytest.mark.gpu

# Worst relative difference between the C oracle's and the numpy loop's iterates over the cases of this file, both on
# the CPU, where the loop ends by the round cap (tests/test_residual_reference_host.py::
# test_refinement_loop_matches_the_oracle re-measures it on every run and holds it under this value); x 16 = four bits
# for the device's different summation orders in sweeps and residuals.
ITERATE_DIFF_MEASURED = 6.6e-16   # edges64 / edges8, caps 1 and 2: 6.3e-16, 6.0e-16, 6.5e-16, 2.7e-16
ITERATE_TOL = 16 * ITERATE_DIFF_MEASURED

WORST = Worst("refinement drivers: true residual / (abstol + bound)")
_S = {}


def setup(name, **over):
    """(ks, K, host factor) for a builder's problem under the refinement settings (+ overrides), once per session."""
    key = (name, tuple(sorted(over.items())))
    if key not in _S:
        from cuclarabel_amd import _lib
        from cuclarabel_amd.kktsolver import HipKKTSolver
        case = rr.refinement_case(name, 1)
        ks = HipKKTSolver(case["P"], case["A"], case["cones"], settings=_lib.default_settings(**dict(case["settings"], **over)))
        assert ks.kktsolver_update(case["hs"])
        assert ks.diagonal_regularizer == rr.REG_EPS
        K = rr.sym_of(ks)
        rr.check_shape(K, case["spec"]["want"])
        fac = _S.get(("factor", name)) or rr.HostFactor(K, ks.maps()["dsigns"], rr.REG_EPS)
        _S[("factor", name)] = fac
        _S[key] = (ks, K, fac, case)
    return _S[key]


def predict(name, B, abstol, max_iter=20):
    ks, K, fac, case = setup(name)
    preds = [rr.refine_loop(K, fac, B[:, j], abstol, 0.0, 5.0, max_iter) for j in range(B.shape[1])]
    lead = preds[0]
    assert lead["norms"][0] >= 1e4 * abstol, ("the first residual must need refinement by 1e4", lead["norms"], abstol)
    for j, p in enumerate(preds):
        assert p["ok"] and p["margin"] >= 4.0, ("a decision too close to its threshold", name, j, p["margin"], p["norms"])
    return preds


def check_columns(tag, name, B, X, ir, abstol, preds, K):
    """(a), (b), (d) for the columns of one call."""
    for j, p in enumerate(preds):
        where = f"{tag} column {j} norms {['%.1e' % v for v in p['norms']]}"
        if ir is not None:
            assert int(ir[j]) == p["rounds"], (where, int(ir[j]), p["rounds"])
        if not np.any(B[:, j]):
            assert not np.any(X[:, j]), (where, "zero column")
            continue
        if p["stop"] == "tol":
            hi, lo = rr.residual_exact(K, X[:, j], B[:, j])
            true = np.abs(hi).max()
            limit = abstol + rr.residual_bound(K, X[:, j], B[:, j]).max()
            WORST.add({name: float(true / limit)}, where)
            assert true <= limit, (where, true, limit)
    print(f"\n[refinement] {tag}: rounds {[p['rounds'] for p in preds]} device {None if ir is None else [int(v) for v in ir]}")


def oracle_rounds(name, B, ks, abstol, max_iter=20):
    from tests import oracle_bindings as ob
    case = rr.refinement_case(name, 1)
    o = ob.OracleKKT(case["P"], case["A"], case["cones"], perm=ks.perm(),
                     settings=ob.default_settings(**dict(case["oracle_settings"], ir_abstol=abstol, ir_max_iter=max_iter)))
    assert o.kktsolver_update_values(case["hs"], [], [], [])
    n = ks.n
    out = []
    for j in range(B.shape[1]):
        o.kktsolver_setrhs(B[:n, j], B[n:, j])
        ok, x, z = o.kktsolver_solve()
        assert ok
        out.append((o.last_ir_iters, np.concatenate([x, z])))
    return out


def solve_multi(ks, B):
    ok, LX, LZ, ir = ks.kktsolver_solve_multi(B[:ks.n], B[ks.n:])
    assert ok
    return np.vstack([LX, LZ]), ir


def solve_single(ks, b):
    ks.kktsolver_setrhs(b[:ks.n], b[ks.n:])
    x, z = np.zeros(ks.n), np.zeros(ks.m)
    assert ks.kktsolver_solve(x, z)
    return np.concatenate([x, z]), ks.last_ir_iterations


# ------------------------------------------------------------------------------------------------ kkt_solve_core
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("name", ["edges64", "edges8"], ids=["partials-mode", "long-row-finishing-kernel"])
def test_solve_core_columns(name, k):
    """1 column through kktsolver_solve (nr = 1); 2, 3 (padded to 4 by a zero column), 4, 5 (4 + 1) and 8 (4 + 4) through
    kktsolver_solve_multi.  edges64 has no long row (k_ir_round reduces the partial maxima), edges8 has four (finishing
    kernels)."""
    ks, K, fac, case = setup(name)
    f = rr.shape_facts(K)
    assert (f["nlong"] == 0) == (name == "edges64")
    abstol = case["abstol"]
    B = rr.refinement_columns(ks.N, k, 50 + k)
    preds = predict(name, B, abstol)
    if k >= 5:
        assert len({p["rounds"] for p in preds}) >= 3        # different counts in one call
    if k == 1:
        x, r = solve_single(ks, B[:, 0])
        X, ir = x[:, None], [r]
    else:
        X, ir = solve_multi(ks, B)
    check_columns(f"core-{name}-nrhs{k}", name, B, X, ir, abstol, preds, K)
    orc = oracle_rounds(name, B, ks, abstol)
    assert [r for r, _ in orc] == [p["rounds"] for p in preds]


@pytest.mark.parametrize("name", ["edges64", "edges8"])
def test_speculation_does_not_change_the_result(name):
    """hipkkt_kkt_speculative_rounds 0, the exact count and more than it: x and the rounds are identical."""
    ks, K, fac, case = setup(name)
    B = rr.refinement_columns(ks.N, 4, 54)
    preds = predict(name, B, case["abstol"])
    most = max(p["rounds"] for p in preds)
    assert most >= 2
    got = []
    for depth in (0, most, most + 3):
        assert ks.speculative_rounds(depth) == depth
        x1, r1 = solve_single(ks, B[:, 0])
        assert ks.speculative_rounds(depth) == depth
        X, ir = solve_multi(ks, B)
        got.append((x1, r1, X, [int(v) for v in ir]))
    for g in got[1:]:
        assert g[1] == got[0][1] == preds[0]["rounds"] and g[3] == got[0][3] == [p["rounds"] for p in preds]
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[2], got[0][2])


@pytest.mark.parametrize("name", ["edges64", "edges8"])
def test_deferred_status_reports_incomplete_refinement(name):
    """Deferred-status mode: a solve runs max(depth, 1) rounds ahead and decides nothing on the host; the status query
    says REFINEMENT_INCOMPLETE exactly when that was fewer than the rounds some column needs."""
    import torch
    from cuclarabel_amd import _lib
    ks, K, fac, case = setup(name)
    B = rr.refinement_columns(ks.N, 4, 54)
    preds = predict(name, B, case["abstol"])
    most = max(p["rounds"] for p in preds)
    assert most >= 2
    dev = torch.device("cuda")
    drx = torch.from_numpy(np.ascontiguousarray(B[:ks.n].T)).to(dev)
    drz = torch.from_numpy(np.ascontiguousarray(B[ks.n:].T)).to(dev)
    dlx = torch.zeros((4, ks.n), dtype=torch.float64, device=dev)
    dlz = torch.zeros((4, ks.m), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ks.set_deferred_status(True)
    try:
        for depth in (0, 1, most, most + 2):
            ks.speculative_rounds(depth)
            ok, ir = ks.kktsolver_solve_multi_dev(4, drx.data_ptr(), drz.data_ptr(), dlx.data_ptr(), dlz.data_ptr())
            status = ks.deferred_status()
            want = _lib.REFINEMENT_INCOMPLETE if max(depth, 1) < most else _lib.OK
            assert ok and status == want, (name, depth, most, status)
            if status == _lib.OK:
                X = np.vstack([dlx.cpu().numpy().T, dlz.cpu().numpy().T])
                check_columns(f"deferred-{name}-depth{depth}", name, B, X, None, case["abstol"], preds, K)
    finally:
        ks.set_deferred_status(False)
        ks.speculative_rounds(0)


# ------------------------------------------------------------------------------------------------ many columns
@pytest.mark.parametrize("k", [9, 10], ids=["nrhs9-NC1", "nrhs10-NC2"])
def test_solve_multi_core_column_major(k):
    """kkt_solve_multi_core: 9 or more columns on a K with long rows; an odd count takes k_residual<G, 1>, an even one
    k_residual<G, 2>; k_accept_columns copies the columns that accept."""
    ks, K, fac, case = setup("edges8")
    assert rr.shape_facts(K)["nlong"] > 0 and k > 8
    B = rr.refinement_columns(ks.N, k, 50 + k)
    preds = predict("edges8", B, case["abstol"])
    X, ir = solve_multi(ks, B)
    check_columns(f"multi-colmajor-nrhs{k}", "edges8", B, X, ir, case["abstol"], preds, K)
    assert [r for r, _ in oracle_rounds("edges8", B, ks, case["abstol"])] == [p["rounds"] for p in preds]


@pytest.mark.parametrize("k,active", [(9, False), (17, True), (64, True)], ids=["nrhs9-KP16", "nrhs17-KP32-swap", "nrhs64-KP64-swap"])
def test_solve_multi_core_row_major(k, active):
    """kkt_solve_multi_core_rm: 9 or more columns, no long rows.  With the zero column (9) some column never accepts and
    every round goes through k_accept_columns_rm; with every column active (17, 64) the first round accepts all columns
    (the buffer swap) and the second only some (the kernel)."""
    ks, K, fac, case = setup("edges64")
    assert rr.shape_facts(K)["nlong"] == 0 and k > 8
    B = rr.refinement_columns(ks.N, k, 50 + k, rr.SCALES_ACTIVE if active else rr.SCALES)
    preds = predict("edges64", B, case["abstol"])
    rounds = [p["rounds"] for p in preds]
    if active:
        assert min(rounds) >= 1 and min(rounds) < max(rounds)      # round 1: all accept; round 2: only some
        assert all(p["norms"][1] < p["norms"][0] / 5 for p in preds)
    else:
        assert min(rounds) == 0 < max(rounds)
    X, ir = solve_multi(ks, B)
    check_columns(f"multi-rowmajor-nrhs{k}", "edges64", B, X, ir, case["abstol"], preds, K)
    if k == 9:
        assert [r for r, _ in oracle_rounds("edges64", B, ks, case["abstol"])] == rounds


# ------------------------------------------------------------------------------------------------ the accept copy's wrap
def test_accept_copy_beyond_one_grid_pass():
    """N = 320 002 > 304 x 256 x 4: the accept copy inside k_ir_round (partials mode) takes a second pass.  A stale tail
    of x would keep the bare solve's entries: every entry must have moved, and the true residual must meet the rule."""
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver
    ks, K, fac, case = setup("accept320k")
    assert ks.N > rr.IR_BLOCKS * 256 * 4 and rr.shape_facts(K)["nlong"] == 0
    B = rr.refinement_columns(ks.N, 1, 51)
    preds = predict("accept320k", B, case["abstol"])
    assert preds[0]["rounds"] >= 1
    x, r = solve_single(ks, B[:, 0])
    check_columns("accept-N320002-nrhs1", "accept320k", B, x[:, None], [r], case["abstol"], preds, K)
    bare = HipKKTSolver(case["P"], case["A"], case["cones"],
                        settings=_lib.default_settings(**dict(case["settings"], iterative_refinement_enable=0)))
    assert bare.kktsolver_update(case["hs"])
    x0, r0 = solve_single(bare, B[:, 0])
    del bare
    assert r0 == 0
    stale = np.flatnonzero(x == x0)
    assert stale.size == 0, (stale.size, stale[:8], stale[-8:])
    assert np.abs(x0 - preds[0]["iterates"][0]).max() <= 1e-9 * np.abs(x0).max()      # it IS the bare solve


# ------------------------------------------------------------------------------------------------ the round cap
@pytest.mark.parametrize("cap", [1, 2])
def test_round_cap(cap):
    """iterative_refinement_max_iter = 1 and 2 with an unreachable tolerance: the loop ends by the cap, rounds = cap, the
    solve succeeds and x is the loop's iterate of that round."""
    abstol = 1e-30
    ks, K, fac, case = setup("edges64", iterative_refinement_max_iter=cap, iterative_refinement_abstol=abstol)
    B = rr.refinement_columns(ks.N, 5, 55)
    preds = [rr.refine_loop(K, fac, B[:, j], abstol, 0.0, 5.0, cap) for j in range(5)]
    for j, p in enumerate(preds):
        assert p["margin"] >= 4.0 and p["stop"] == ("tol" if not np.any(B[:, j]) else "cap"), (j, p["stop"], p["margin"])
    x, r = solve_single(ks, B[:, 0])
    X, ir = solve_multi(ks, B)
    assert r == cap and [int(v) for v in ir] == [p["rounds"] for p in preds] == [cap, cap, 0, cap, cap]
    orc = oracle_rounds("edges64", B, ks, abstol, max_iter=cap)
    assert [v for v, _ in orc] == [p["rounds"] for p in preds]
    for j, p in enumerate(preds):
        scale = np.abs(p["x"]).max()
        if scale == 0.0:
            assert not np.any(X[:, j])
            continue
        assert np.abs(X[:, j] - p["x"]).max() <= ITERATE_TOL * scale, (cap, j, np.abs(X[:, j] - p["x"]).max() / scale)
    assert np.abs(x - preds[0]["x"]).max() <= ITERATE_TOL * np.abs(x).max()


def test_report_worst_ratios():
    WORST.report()
