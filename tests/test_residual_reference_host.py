"""The host reference of the refinement tests (tests/residual_reference.py) checked on its own, without a GPU:

  - the exact residual against mpmath at 60 digits, its error at least 2^10 below the bound it is used with;
  - the builders reach the row lengths, long-row counts, lane widths and sizes their GPU cases are named after;
  - the bound has teeth: each simulated kernel fault (an entry dropped from a long row, a whole chunk dropped, the last
    entry of a row of length 1 mod 8 and mod 64 dropped, an entry counted twice, a neighbouring column's x used for one
    entry) violates it on every builder, while the exact residual rounded to fp64 and a plain fp64 residual pass;
  - the numpy refinement loop takes the rounds the C oracle takes.
"""
import math

import mpmath
import numpy as np
import pytest

from tests import residual_reference as rr

SPECS = {s()["name"]: s for s in (rr.spec_edges8, rr.spec_edges64, rr.spec_long257, rr.spec_wrap70k, rr.spec_accept320k)}
_IMG = {}


def image(name):
    """(K, facts, x, b) of a builder, once per session; x, b with three columns."""
    if name not in _IMG:
        spec = SPECS[name]()
        P, A, cones = rr.make_problem(spec)
        K = rr.expected_image(P, A, rr.hs_values(cones, spec["seed"] + 1))
        facts = rr.check_shape(K, spec["want"])
        x, b = rr.probe_vectors(K.shape[0], 3, spec["seed"] + 2)
        _IMG[name] = (K, facts, x, b)
    return _IMG[name]


def _mp_row(K, x, b, i):
    a, z = K.indptr[i], K.indptr[i + 1]
    s = mpmath.mpf(float(b[i]))
    for v, j in zip(K.data[a:z].tolist(), K.indices[a:z].tolist()):
        s -= mpmath.mpf(v) * mpmath.mpf(float(x[j]))
    return s


@pytest.mark.parametrize("name", ["edges64", "edges8"])
def test_exact_residual_against_mpmath(name):
    K, facts, x, b = image(name)
    x, b = x[:, 0], b[:, 0]
    hi, lo = rr.residual_exact(K, x, b)
    bound = rr.residual_bound(K, x, b)
    L = facts["lengths"]
    rows = range(K.shape[0]) if name == "edges64" else np.flatnonzero((L > 60) | (L < 3)).tolist()
    worst = 0.0
    with mpmath.workdps(60):
        for i in rows:
            ref = _mp_row(K, x, b, i)
            err = abs(ref - (mpmath.mpf(float(hi[i])) + mpmath.mpf(float(lo[i]))))
            assert abs(ref - mpmath.mpf(float(hi[i]))) <= abs(ref) * rr.U, (name, i)          # hi: correctly rounded
            worst = max(worst, float(err / mpmath.mpf(float(bound[i]))))
    assert worst <= 2.0 ** -10, worst                      # the issue's requirement ...
    assert worst <= 2.0 ** -40, worst                      # ... and what the construction gives


def test_sym_from_triu_small():
    # [[1, 2, 0], [2, 0, 3], [0, 3, 4]] with an explicit zero on the diagonal, which must stay structural
    K = rr.sym_from_triu([0, 1, 3, 5], [0, 0, 1, 1, 2], [1.0, 2.0, 0.0, 3.0, 4.0])
    assert np.array_equal(K.toarray(), [[1, 2, 0], [2, 0, 3], [0, 3, 4]])
    assert rr.row_lengths(K).tolist() == [2, 3, 2] and K.indices.tolist() == [0, 1, 0, 1, 2, 1, 2]


@pytest.mark.parametrize("name", list(SPECS))
def test_builders_reach_their_edges(name):
    K, f, _, _ = image(name)
    want = SPECS[name]()["want"]
    assert f["lanes"] == want["lanes"] and f["nlong"] == want["nlong"]
    if name == "edges8":
        L = f["lengths"]
        assert sorted(L[L > rr.LONG_ROW].tolist()) == [4097, 4097, 6144, 6145]
        assert f["nchunks"] == 3 + 3 + 3 + 4               # 4097 = 2 chunks + 1 entry; 6144 = exactly 3 chunks; 6145 = 3 + 1
        assert K.indptr[-1] / f["N"] <= rr.LANE_AVG and f["N"] % 32
    if name == "edges64":
        assert f["N"] % 4 and f["grid"] > 1
    if name == "long257":
        assert f["nlong"] > 256 and (f["lengths"][-257:] == 4201).all()
    if name == "wrap70k":
        assert f["grid_uncapped"] > rr.NORM_PARTS and f["grid"] == rr.NORM_PARTS and f["N"] > rr.RM_BLOCKS * 16
    if name == "accept320k":
        assert f["N"] > rr.IR_BLOCKS * 256 * 4


def _fault_rows(K, fault, L):
    """The rows a fault is tried on: the long rows (the longest row where there is none); for drop_last the rows of
    length 1 mod 8 and mod 64 (65, 129, 4097, 6145) whose last entry is not a structural zero (a zero cone's diagonal:
    dropping it is no fault), or the longest rows with a non-zero last entry where the builder has none of those."""
    if fault == "drop_last":
        live = K.data[K.indptr[1:] - 1] != 0.0
        r = [int(i) for c in (65, 129, 4097, 6145) for i in np.flatnonzero((L == c) & live)[:2]]
        return r or [int(i) for i in np.flatnonzero(live & (L == L[live].max()))[:2]]
    r = np.flatnonzero(L > rr.LONG_ROW)
    return [int(i) for i in r[:4]] if r.size else [int(np.argmax(L))]


@pytest.mark.parametrize("fault", rr.FAULTS)
@pytest.mark.parametrize("name", list(SPECS))
def test_simulated_faults_violate_the_bound(name, fault):
    K, f, x, b = image(name)
    exact = rr.residual_exact(K, x[:, 0], b[:, 0])
    bound = rr.residual_bound(K, x[:, 0], b[:, 0])
    rows = _fault_rows(K, fault, f["lengths"])
    assert rows
    if fault == "drop_last" and name in ("edges8", "edges64"):
        assert {int(f["lengths"][i]) % 64 for i in rows} == {1} and len(rows) >= 2
    for i in rows:
        bad = rr.faulty_residual(K, x[:, 0], b[:, 0], i, fault, x_other=x[:, 1])
        err = abs((bad - exact[0][i]) - exact[1][i])
        assert err > bound[i], (name, fault, i, int(f["lengths"][i]), err, bound[i])
        assert err > 1e3 * bound[i], (name, fault, i, err / bound[i])     # not a near miss either


@pytest.mark.parametrize("name", list(SPECS))
def test_correct_residuals_pass_the_bound(name):
    K, f, x, b = image(name)
    exact = rr.residual_exact(K, x, b)
    bound = rr.residual_bound(K, x, b)
    assert (rr.error_vs_exact(exact[0], exact) <= bound).all()             # the exact residual rounded to fp64
    assert (rr.error_vs_exact(exact[0], exact) <= rr.U * np.abs(exact[0])).all()
    plain = b - K @ x                                                       # one particular summation order
    assert (rr.error_vs_exact(plain, exact) <= bound).all()
    back = np.stack([(b[:, j][::-1] - (K[::-1] @ x[:, j])) for j in range(x.shape[1])], axis=1)[::-1]
    assert (rr.error_vs_exact(back, exact) <= bound).all()


def test_margin_and_loop_bookkeeping():
    assert rr.margin(8.0, 2.0) == 4.0 and rr.margin(2.0, 8.0) == 4.0 and rr.margin(0.0, 1.0) == math.inf
    # a "factor" that gains exactly one digit per round: 0.1 -> 0.01 -> 0.001; the loop stops by tolerance after 2 rounds
    K = rr.sym_from_triu([0, 1], [0], [1.0])
    out = rr.refine_loop(K, lambda r: 0.9 * r, np.array([1.0]), 2e-3, 0.0, 5.0, 20)
    assert out["rounds"] == 2 and out["stop"] == "tol" and np.allclose(out["norms"], [1e-1, 1e-2, 1e-3])
    assert 1.9 < out["margin"] < 2.1                                        # 2e-3 / 1e-3, and the ratio 10 against 5
    out = rr.refine_loop(K, lambda r: 0.9 * r, np.array([1.0]), 0.0, 0.0, 5.0, 2)
    assert out["rounds"] == 2 and out["stop"] == "cap" and len(out["iterates"]) == 3
    out = rr.refine_loop(K, lambda r: 6.0 * r, np.array([1.0]), 0.0, 0.0, 5.0, 20)      # diverges: 5 -> 25
    assert out["rounds"] == 1 and out["stop"] == "ratio" and not out["accepted_last"] and out["x"][0] == 6.0
    out = rr.refine_loop(K, lambda r: r, np.array([0.0]), 1e-12, 0.0, 5.0, 20)
    assert out["rounds"] == 0 and out["stop"] == "tol" and out["x"][0] == 0.0


@pytest.mark.parametrize("cap", [1, 2, 20])
@pytest.mark.parametrize("name", ["edges64", "edges8"])
def test_refinement_loop_matches_the_oracle(name, cap):
    """Rounds per column of the numpy loop = those of the C oracle (oracle/kkt_oracle.c: its own LDL' and residual) on the
    refinement tests' problems and settings, every decision clear of its threshold by 4 x; and the iterates agree within
    ITERATE_TOL = 16 x the worst difference measured here (printed under -s; the constant sits in test_gpu_refinement.py)."""
    from tests import oracle_bindings as ob
    from tests.test_gpu_refinement import ITERATE_DIFF_MEASURED, ITERATE_TOL
    case = rr.refinement_case(name, 10)
    abstol = case["abstol"] if cap == 20 else 1e-30
    o = ob.OracleKKT(case["P"], case["A"], case["cones"],
                     settings=ob.default_settings(**dict(case["oracle_settings"], ir_abstol=abstol, ir_max_iter=cap)))
    assert o.kktsolver_update_values(case["hs"], [], [], [])
    M = o.K()
    K = rr.sym_from_triu(M.indptr, M.indices, M.data)
    rr.check_shape(K, case["spec"]["want"])
    solve = rr.HostFactor(K, o.dsigns(), case["eps"])
    n = case["P"].shape[0]
    worst = 0.0
    for j in range(case["B"].shape[1]):
        bj = case["B"][:, j]
        pred = rr.refine_loop(K, solve, bj, abstol, 0.0, 5.0, cap)
        o.kktsolver_setrhs(bj[:n], bj[n:])
        ok, x, z = o.kktsolver_solve()
        assert ok and o.last_ir_iters == pred["rounds"], (j, o.last_ir_iters, pred["rounds"], pred["norms"])
        assert pred["margin"] >= 4.0, (j, pred["margin"], pred["norms"])
        scale = np.abs(pred["x"]).max()
        if scale:
            worst = max(worst, np.abs(np.concatenate([x, z]) - pred["x"]).max() / scale)
    print(f"\n[refinement host] {name} cap {cap}: oracle vs numpy loop, worst relative iterate difference {worst:.3e}")
    if cap < 20:            # the comparison is made where the loop ends by the cap (test_gpu_refinement.test_round_cap)
        assert worst <= ITERATE_DIFF_MEASURED, (worst, ITERATE_DIFF_MEASURED)
    assert ITERATE_TOL == 16 * ITERATE_DIFF_MEASURED
