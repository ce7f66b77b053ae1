"""Ruiz equilibration: the numpy restatement against the reference's own unit tests
(test/UnitTests/test_equilibration_bounds.jl) on CPU, and the device routine against the restatement on GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import problems
from cuclarabel_amd.cones import NonnegativeConeT
from tests.ref_equilibrate_numpy import equilibrate_ref


def reference_test_data():
    """test_equilibration_bounds.jl:6-20"""
    P = sp.csc_matrix(np.array([[4.0, 1.0], [1.0, 2.0]]))
    c = np.array([1.0, 1.0])
    A = np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    l, u = np.array([1.0, 0.0, 0.0]), np.array([1.0, 0.7, 0.7])
    A = sp.csc_matrix(np.vstack([-A, A]))
    b = np.concatenate([-l, u])
    return P, c, A, b, [NonnegativeConeT(3), NonnegativeConeT(3)]


def _bounds_ok(d, e, lo=1e-4, hi=1e4):
    return d.min() >= lo and e.min() >= lo and d.max() <= hi and e.max() <= hi


def _variants():
    P, c, A, b, cones = reference_test_data()
    Pl = P.tolil(); Pl[0, 0] = 1e-15                       # "equilibrate lower bound" (:28-43)
    Au = A.tolil(); Au[0, 0] = 1e15                        # "equilibrate upper bound" (:45-61)
    Az = A.copy(); Az.data[:] = 0.0                        # "equilibrate zero rows" (:63-76)
    return {"lower": (Pl.tocsc(), c, A, b, cones), "upper": (P, c, Au.tocsc(), b, cones), "zero_rows": (P, c, Az, b, cones)}


@pytest.mark.parametrize("name", ["lower", "upper", "zero_rows"])
def test_restatement_meets_the_reference_unit_tests(name):
    P, c, A, b, cones = _variants()[name]
    _, _, _, _, d, e, _ = equilibrate_ref(P, c, A, b, cones)
    assert _bounds_ok(d, e)
    if name == "zero_rows":
        assert np.all(e == 1.0)


def test_restatement_scales_consistently():
    pb = problems.small_mixed(seed=3)
    Ps, qs, As, bs, d, e, c = equilibrate_ref(pb.P, pb.q, pb.A, pb.b, pb.cones)
    Pt = sp.triu(sp.csc_matrix(pb.P))
    np.testing.assert_allclose(Ps.toarray(), c * (np.diag(d) @ Pt.toarray() @ np.diag(d)), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(As.toarray(), np.diag(e) @ pb.A.toarray() @ np.diag(d), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(qs, c * d * pb.q, rtol=1e-12)
    np.testing.assert_allclose(bs, e * pb.b, rtol=1e-12)
    # cones without elementwise scaling carry one factor each
    off = 0
    for cone in pb.cones:
        if not isinstance(cone, NonnegativeConeT) and type(cone).__name__ != "ZeroConeT":
            assert np.ptp(e[off:off + cone.numel]) <= 1e-15 * e[off]
        off += cone.numel


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lower", "upper", "zero_rows"])
def test_device_equilibration_on_the_reference_unit_tests(name):
    from cuclarabel_amd.equilibrate import equilibrate
    P, c, A, b, cones = _variants()[name]
    Ps, qs, As, bs, eq = equilibrate(P, c, A, b, cones)
    assert _bounds_ok(eq.d, eq.e)
    if name == "zero_rows":
        assert np.all(eq.e == 1.0)
    Pr, qr, Ar, br, d, e, cc = equilibrate_ref(P, c, A, b, cones)
    np.testing.assert_allclose(eq.d, d, rtol=1e-13)
    np.testing.assert_allclose(eq.e, e, rtol=1e-13)
    assert eq.c == pytest.approx(cc, rel=1e-13)


@pytest.mark.gpu
@pytest.mark.parametrize("maker", [lambda: problems.small_mixed(seed=3), lambda: problems.config1(),
                                   lambda: problems.config2(n=3000), lambda: problems.config5(n=300, npsd=5, psd_dim=6, nsoc=3, soc_dim=9)],
                         ids=["mixed", "cfg1", "cfg2_n3000", "cfg5_small"])
def test_device_equilibration_matches_restatement(maker):
    from cuclarabel_amd.equilibrate import equilibrate, rescale_A, rescale_P
    pb = maker()
    Ps, qs, As, bs, eq = equilibrate(pb.P, pb.q, pb.A, pb.b, pb.cones)
    Pr, qr, Ar, br, d, e, c = equilibrate_ref(pb.P, pb.q, pb.A, pb.b, pb.cones)
    # the only order-dependent quantity is the mean column norm of P (a sum): a few ulp
    np.testing.assert_allclose(eq.d, d, rtol=1e-12)
    np.testing.assert_allclose(eq.e, e, rtol=1e-12)
    assert eq.c == pytest.approx(c, rel=1e-12)
    np.testing.assert_array_equal(Ps.indices, Pr.indices)
    np.testing.assert_allclose(Ps.data, Pr.data, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(As.data, Ar.data, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(qs, qr, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(bs, br, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(eq.dinv * eq.d, 1.0, rtol=1e-15)
    # update_P! / update_A! re-scaling of fresh data reproduces the scaled matrices
    np.testing.assert_allclose(rescale_P(pb.P, eq).data, Ps.data, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(rescale_A(pb.A, eq).data, As.data, rtol=1e-12, atol=1e-300)
    # no scaling requested: identity
    P0, q0, A0, b0, eq0 = equilibrate(pb.P, pb.q, pb.A, pb.b, pb.cones, max_iter=0)
    assert np.all(eq0.d == 1.0) and np.all(eq0.e == 1.0) and eq0.c == 1.0
    np.testing.assert_array_equal(A0.data, sp.csc_matrix(pb.A).data)


@pytest.mark.gpu
def test_equilibrated_problem_solves_to_the_same_point():
    """Solving the scaled problem and un-scaling (x = D x~, solution_post_process!) gives the solution of
    the original one: the basic QP of the reference's tests."""
    from cuclarabel_amd import ipm
    from cuclarabel_amd.equilibrate import equilibrate
    from tests.golden import reference_fixtures as fx
    P, q, A, b, cones, exp = fx.basic_qp()
    Ps, qs, As, bs, eq = equilibrate(P, q, A, b, cones)
    res = ipm.solve(Ps, qs, As, bs, cones, ipm.HipBackend(Ps, As, cones))
    assert res.status == "SOLVED"
    np.testing.assert_allclose(res.x * eq.d, exp["x"], atol=1e-3)


# ================================================================================================ kernel edges
# k_equil_rectify is one wave per cone with a 64-stride loop; k_equil_cost_partials is capped at 256 workgroups of 256;
# k_equil_norms / _scale_data / k_lrscale at 4096 workgroups of 256.  The problems below sit on those edges.  The reference
# stays equilibrate_ref with this file's rtol = 1e-12 ("same order except the one sum"); k_lrscale's three products have
# one correct answer each and are compared byte for byte.
RTOL = 1e-12


def _rng_problem(n, cones, seed, density=0.2, decades=6.0):
    """(P, q, A, b): A random with every row non-empty and the rows scaled over `decades` decades, P sparse symmetric"""
    rng = np.random.default_rng(seed)
    m = sum(c.numel for c in cones)
    A = sp.random(m, n, density=density, random_state=np.random.RandomState(seed), format="lil")
    for i in range(m):
        A[i, i % n] = 1.0 + rng.random()
    A = sp.csc_matrix(sp.diags(10.0 ** rng.uniform(-decades / 2, decades / 2, m)) @ sp.csc_matrix(A))
    G = sp.random(n, n, density=0.1, random_state=np.random.RandomState(seed + 1), format="csc")
    P = sp.triu(sp.csc_matrix(G @ G.T + sp.identity(n)), format="csc")
    return P, rng.standard_normal(n), A, rng.standard_normal(m)


def rectify_cones():
    from cuclarabel_amd.cones import (ZeroConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT, GenPowerConeT)
    return [SecondOrderConeT(63), SecondOrderConeT(64), SecondOrderConeT(65), SecondOrderConeT(129), PSDTriangleConeT(48),
            SecondOrderConeT(1), NonnegativeConeT(5), ZeroConeT(3), GenPowerConeT(problems.normalised_alphas(np.ones(40)), 60),
            ExponentialConeT()]


def rectify_problem():
    cones = rectify_cones()
    assert [c.numel for c in cones] == [63, 64, 65, 129, 1176, 1, 5, 3, 100, 3]
    return _rng_problem(40, cones, 6101) + (cones,)


def many_soc_problem():
    from cuclarabel_amd.cones import SecondOrderConeT
    cones = [SecondOrderConeT(5) for _ in range(300)]
    return _rng_problem(30, cones, 6102, density=0.1) + (cones,)


def cost_problem(n, where, decides="q"):
    """P diagonal, A one entry per row; the largest |q| and the largest column norm of P both at the first or last index.
    decides: which half of k_equil_cost_partials sets c -- "q": |q|_inf = 100 (the maximum), "P": q of order 1e-3, so the
    mean column norm of P (the sum, block by block and across the grid stride) does."""
    rng = np.random.default_rng(6200 + n)
    i = 0 if where == "first" else n - 1
    p = rng.uniform(0.5, 1.5, n)
    q = rng.standard_normal(n) * (1.0 if decides == "q" else 1e-4)
    p[i], q[i] = 50.0, (-100.0 if decides == "q" else -1e-3)
    if n == 1 and decides == "P":
        p[0] = 0.3                                          # (below |A[0, 0]|: the one scaled column norm is not 1, so c != 1)
    A = sp.diags(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n), format="csc")
    assert np.argmax(p) == i == np.argmax(np.abs(q))
    return sp.diags(p, format="csc"), q, A, rng.standard_normal(n), [NonnegativeConeT(n)]


def first_round_cost_terms(P, q, A, b, cones):
    """(mean column norm of P, |q|_inf) as the first round's cost scaling saw them, up to the common factor it applied"""
    Ps, qs = equilibrate_ref(P, q, A, b, cones, max_iter=1)[:2]
    cn = np.zeros(Ps.shape[0])
    np.maximum.at(cn, np.repeat(np.arange(Ps.shape[0]), np.diff(Ps.indptr)), np.abs(Ps.data))
    return cn.mean(), np.abs(qs).max()


COST_N = (1, 255, 256, 257, 65_536 + 257)


def lp_problem():
    cones = [NonnegativeConeT(30)]
    P, q, A, b = _rng_problem(12, cones, 6301, decades=2.0)
    return sp.csc_matrix((12, 12)), q, A, b, cones


def zero_q_problem():
    cones = [NonnegativeConeT(30)]
    P, q, A, b = _rng_problem(12, cones, 6302, decades=2.0)
    return P, np.zeros(12), A, b, cones


def no_constraints_problem():
    P, q, _, _ = _rng_problem(12, [NonnegativeConeT(1)], 6303)
    return P, q, sp.csc_matrix((0, 12)), np.zeros(0), []


ZERO_COLUMNS = (3, 7)


def zero_column_problem():
    """column 3 of P and A structurally empty, column 7 stored with zero values"""
    cones = [NonnegativeConeT(30)]
    P, q, A, b = _rng_problem(12, cones, 6304, decades=2.0)
    Pc, Ac = sp.triu(P, format="coo"), A.tocoo()
    keep = (Pc.row != 3) & (Pc.col != 3)
    pv = np.where((Pc.row == 7) | (Pc.col == 7), 0.0, Pc.data)
    P = sp.csc_matrix((pv[keep], (Pc.row[keep], Pc.col[keep])), shape=P.shape)
    keep = Ac.col != 3
    av = np.where(Ac.col == 7, 0.0, Ac.data)
    A = sp.csc_matrix((av[keep], (Ac.row[keep], Ac.col[keep])), shape=A.shape)
    P.sort_indices(); A.sort_indices()
    assert P.indptr[8] > P.indptr[7] and A.indptr[8] > A.indptr[7] and P.indptr[4] == P.indptr[3] and A.indptr[4] == A.indptr[3]
    return P, q, A, b, cones


def banded_big_problem():
    from tests.kvalue_reference import banded_big_data
    P, A = banded_big_data()
    rng = np.random.default_rng(6401)
    n = A.shape[0]
    assert P.nnz + A.nnz > 4096 * 256 and n > 65_536
    return P, rng.standard_normal(n), A, rng.standard_normal(n), [NonnegativeConeT(n)]


NEW_PROBLEMS = {"rectify": rectify_problem, "many_soc": many_soc_problem, "lp": lp_problem, "zero_q": zero_q_problem,
                "no_constraints": no_constraints_problem, "zero_column": zero_column_problem, "banded_big": banded_big_problem,
                **{f"cost[{n},{w}]": (lambda n=n, w=w: cost_problem(n, w)) for n in COST_N for w in ("first", "last")},
                **{f"cost[{n},{w},P]": (lambda n=n, w=w: cost_problem(n, w, "P")) for n in COST_N for w in ("first", "last")}}
_REF = {}


def new_problem(name, max_iter=10):
    """(problem, the reference's result): computed once and shared"""
    if (name, max_iter) not in _REF:
        pb = NEW_PROBLEMS[name]()
        _REF[(name, max_iter)] = (pb, equilibrate_ref(*pb, max_iter=max_iter))
    return _REF[(name, max_iter)]


def _rows_of(cones):
    off = 0
    for cone in cones:
        yield cone, slice(off, off + cone.numel)
        off += cone.numel


def _scalar_cones(cones):
    return [(c, r) for c, r in _rows_of(cones) if not isinstance(c, NonnegativeConeT) and type(c).__name__ != "ZeroConeT"]


@pytest.mark.parametrize("name", sorted(NEW_PROBLEMS))
def test_restatement_handles_the_edge_problems(name):
    (P, q, A, b, cones), (Ps, qs, As, bs, d, e, c) = new_problem(name)
    for v in (Ps.data, qs, As.data, bs, d, e, [c]):
        assert np.isfinite(v).all()
    assert _bounds_ok(d, e if e.size else np.ones(1)) and 1e-4 <= c <= 1e4
    for cone, r in _scalar_cones(cones):
        assert np.ptp(e[r]) <= 1e-15 * e[r][0]
    if name == "lp":
        assert c == 1.0 and Ps.nnz == 0
    if name == "zero_q":
        assert c == 1.0
    if name == "no_constraints":
        assert e.size == 0 and As.shape == (0, 12) and (d != 1.0).any()
    if name == "zero_column":
        assert (d[list(ZERO_COLUMNS)] == 1.0).all() and (np.delete(d, ZERO_COLUMNS) != 1.0).all()
    if name.startswith("cost"):
        mean_p, nq = first_round_cost_terms(P, q, A, b, cones)
        assert c != 1.0 and ((mean_p > 10 * nq) if name.endswith(",P]") else (nq > 10 * mean_p))


@pytest.mark.parametrize("name", ["rectify", "many_soc"])
def test_rectify_problems_vary_inside_every_cone_before_rectification(name):
    """with every row on a nonnegative cone nothing is rectified: e then spreads over decades inside each cone"""
    P, q, A, b, cones = new_problem(name)[0]
    e = equilibrate_ref(P, q, A, b, [NonnegativeConeT(A.shape[0])])[5]
    over64 = 0
    for cone, r in _scalar_cones(cones):
        if cone.numel > 1:
            assert e[r].max() > 3.0 * e[r].min(), (type(cone).__name__, cone.numel)
        over64 += cone.numel > 64
    assert over64 >= (4 if name == "rectify" else 0)         # SOC(65), SOC(129), PSD(48), the generalized power cone


# ------------------------------------------------------------------------------------------------ GPU
def _device_vs_reference(name, max_iter=10):
    from cuclarabel_amd.equilibrate import equilibrate
    (P, q, A, b, cones), (Pr, qr, Ar, br, d, e, c) = new_problem(name, max_iter)
    Ps, qs, As, bs, eq = equilibrate(P, q, A, b, cones, max_iter=max_iter)
    np.testing.assert_allclose(eq.d, d, rtol=RTOL)
    np.testing.assert_allclose(eq.e, e, rtol=RTOL)
    assert eq.c == pytest.approx(c, rel=RTOL)
    np.testing.assert_array_equal(Ps.indices, Pr.indices)
    np.testing.assert_allclose(Ps.data, Pr.data, rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(As.data, Ar.data, rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(qs, qr, rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(bs, br, rtol=RTOL, atol=1e-300)
    return (P, q, A, b, cones), (Ps, qs, As, bs, eq)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rectify", "many_soc"])
def test_device_rectification_past_one_wave_stride(name):
    (P, q, A, b, cones), (Ps, qs, As, bs, eq) = _device_vs_reference(name)
    sizes = [c.numel for c, _ in _scalar_cones(cones)]
    assert (max(sizes) == 1176 and {65, 129, 100} <= set(sizes)) if name == "rectify" else sizes == [5] * 300
    for cone, r in _scalar_cones(cones):
        assert np.ptp(eq.e[r]) <= 1e-15 * eq.e[r][0], (type(cone).__name__, cone.numel)


@pytest.mark.gpu
@pytest.mark.parametrize("decides", ["q", "P"])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", COST_N)
def test_device_cost_scaling_at_the_partials_edges(n, where, decides):
    """c from the maximum of |q| (decides = q) and from the SUM of P's column norms (decides = P: one dropped term of the
    sum moves c by 1 / n, far outside 1e-12)"""
    assert n in (1, 255, 256, 257) or n > 256 * 256
    name = f"cost[{n},{where}]" if decides == "q" else f"cost[{n},{where},P]"
    pb = new_problem(name)[0]
    mean_p, nq = first_round_cost_terms(*pb)
    assert (mean_p > 10 * nq) if decides == "P" else (nq > 10 * mean_p)
    _, (Ps, qs, As, bs, eq) = _device_vs_reference(name)
    assert eq.c != 1.0


@pytest.mark.gpu
def test_device_degenerate_data():
    _, (Ps, qs, As, bs, eq) = _device_vs_reference("lp")
    assert eq.c == 1.0 and Ps.nnz == 0
    _, (Ps, qs, As, bs, eq) = _device_vs_reference("zero_q")
    assert eq.c == 1.0 and not qs.any()
    _, (Ps, qs, As, bs, eq) = _device_vs_reference("no_constraints")
    assert eq.e.size == 0 and As.nnz == 0 and (eq.d != 1.0).any()
    _, (Ps, qs, As, bs, eq) = _device_vs_reference("zero_column")
    assert (eq.d[list(ZERO_COLUMNS)] == 1.0).all()
    _device_vs_reference("rectify", max_iter=1)


@pytest.mark.gpu
def test_device_equilibration_past_the_grid_cap():
    (P, q, A, b, cones), _ = _device_vs_reference("banded_big")
    assert P.nnz + A.nnz > 4096 * 256


def _lr_expected(M, L, R, c):
    M = sp.csc_matrix(M)
    col = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    return M.data * (L[M.indices] * R[col]) * c


def _P_with_nnz(nnz, rng):
    n = (nnz + 1) // 2 if nnz % 2 else nnz
    P = sp.diags(rng.uniform(0.5, 1.5, n), format="csc")
    if nnz % 2 and n > 1:
        P = (P + sp.diags(rng.standard_normal(n - 1), 1, format="csc")).tocsc()
    assert P.nnz == nnz
    return P


@pytest.mark.gpu
@pytest.mark.parametrize("nnz", [1, 255, 256, 257, "banded_big"])
def test_rescaled_values_are_three_correctly_rounded_products(nnz):
    """k_lrscale: v * (L[row] * R[col]) * c in that order, no contraction: one answer, compared byte for byte"""
    from cuclarabel_amd.equilibrate import Equilibration, rescale_A, rescale_P
    rng = np.random.default_rng(6500)
    if nnz == "banded_big":
        P, _, A, _, _ = new_problem("banded_big")[0]
        assert A.nnz > 4096 * 256
    else:
        P = _P_with_nnz(nnz, rng)
        A = sp.csc_matrix(sp.coo_matrix((rng.standard_normal(nnz), (np.arange(nnz), np.arange(nnz) % 3)), shape=(nnz, 3)))
        A = sp.hstack([A, sp.csc_matrix((nnz, P.shape[0] - 3))], format="csc") if P.shape[0] > 3 else A[:, :P.shape[0]]
        A = sp.csc_matrix(A)
        A.sort_indices()
        assert nnz < 3 or A.nnz == nnz
    n, m = P.shape[0], A.shape[0]
    d, e = np.exp(rng.standard_normal(n)), np.exp(rng.standard_normal(m))
    eq = Equilibration(d, 1.0 / d, e, 1.0 / e, 0.37)
    got = rescale_P(P, eq)
    assert got.data.tobytes() == _lr_expected(sp.triu(P, format="csc"), d, d, 0.37).tobytes()
    got = rescale_A(A, eq)
    assert got.data.tobytes() == _lr_expected(A, e, d, 1.0).tobytes()


@pytest.mark.gpu
def test_rescale_of_an_empty_matrix_and_one_based_indices():
    import ctypes as C
    from cuclarabel_amd import _lib
    from cuclarabel_amd.equilibrate import _scale_values
    rng = np.random.default_rng(6501)
    L, R = np.exp(rng.standard_normal(5)), np.exp(rng.standard_normal(4))
    empty = _scale_values(sp.csc_matrix((5, 4)), L, R, 0.37)
    assert empty.nnz == 0 and empty.shape == (5, 4)
    M = sp.random(5, 4, density=0.6, random_state=np.random.RandomState(3), format="csc")
    M.sort_indices()
    want = _lr_expected(M, L, R, 0.37)
    assert _scale_values(M, L, R, 0.37).data.tobytes() == want.tobytes()
    cp, ri, v = _lib.i64(M.indptr) + 1, _lib.i64(M.indices) + 1, _lib.f64(M.data).copy()
    rc = _lib.lib().hipkkt_scale_matrix_values(5, 4, _lib.ptr(cp), _lib.ptr(ri), _lib.ptr(v), _lib.ptr(L), _lib.ptr(R),
                                               C.c_double(0.37), 1, -1)
    assert rc == 0 and v.tobytes() == want.tobytes()
