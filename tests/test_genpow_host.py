"""The generalized power cone on the host: ipm._GenPow against the extended-precision derivatives of the dual barrier,
gradient_primal by its defining conditions, the expanded K of tests/genpow_reference.py against the reduced dense
system, the reference's known answer through the IPM driver on a scipy backend, and the constructor's validation."""
import numpy as np
import pytest
import mpmath as mp

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import (GenPowerConeT, PowerConeT, SecondOrderConeT, ZeroConeT, NonnegativeConeT, KIND_GENPOW,
                                  cone_param_ptr_vals, cone_params, has_nonsymmetric)
from tests import genpow_reference as G
from tests.golden import genpow_fixtures as F
from tests.golden import nonsymmetric_fixtures as FN

# float64 closed forms against 60-digit values: a few hundred roundings at most (the running product over dim1, the sum
# over dim2, a dozen operations behind them), each 1.1e-16, amplified by phi / zeta <= 1 / (1 - 0.9^2) ~ 5.3 where
# zeta = phi - ||w||^2 cancels (random_interior_pair keeps ||w|| under 0.9 of its bound)
def _tol(spec):
    return 5.3 * (spec.dim + 16) * 2.3e-16


def _points(shapes, seed, per_shape=2):
    rng = np.random.default_rng(seed)
    out = []
    for d1, d2 in shapes:
        spec = G.random_spec(rng, d1, d2)
        for j in range(per_shape):
            out.append((spec,) + (G.random_interior_pair(spec, rng) if j % 2 == 0 else G.central_pair(spec, rng)))
    return out


def _host(spec, z, mu=1.0):
    c = ipm._make_cones([spec])[0]
    assert c.update_scaling(z.copy(), z.copy(), mu, ipm.DUAL)
    return c


@pytest.mark.parametrize("spec,s,z", _points(G.SHAPES, 5))
def test_grad_and_hessian_equal_the_derivatives_of_the_dual_barrier(spec, s, z):
    c = _host(spec, z)
    g_mp, H_mp = G.mp_grad(spec, z), G.mp_hess(spec, z)
    assert G.rel_err(c.grad, g_mp) <= _tol(spec)
    H = c.H_dual
    scale = max(abs(H_mp[i, j]) for i in range(c.n) for j in range(c.n))
    err = max(abs(mp.mpf(float(H[i, j])) - H_mp[i, j]) for i in range(c.n) for j in range(c.n)) / scale
    # D + pp' - qq' - rr' cancels: its terms are up to (phi + ||w||^2) / zeta <= 9.6 times the entries of H
    assert float(err) <= 9.6 * _tol(spec)
    # the 60-digit closed forms the device tests measure against are the same derivatives
    gc, d, p, q, r = G.mp_closed(spec, z)
    Hc = G.mp_dense_H(d, p, q, r)
    assert max(abs(gc[i] - g_mp[i]) for i in range(c.n)) <= mp.mpf(10) ** -30 * max(abs(v) for v in g_mp)
    assert max(abs(Hc[i, j] - H_mp[i, j]) for i in range(c.n) for j in range(c.n)) <= mp.mpf(10) ** -25 * scale


@pytest.mark.parametrize("spec,s,z", _points(G.BIG_SHAPES, 6, per_shape=1))
def test_grad_and_hessian_along_directions_for_cones_of_hundreds_of_rows(spec, s, z):
    c = _host(spec, z)
    rng = np.random.default_rng(spec.dim)
    H = c.H_dual
    for _ in range(2):
        v, w = rng.standard_normal(c.n), rng.standard_normal(c.n)
        g_mp, h_mp = G.mp_directional(spec, z, v, w)
        gs = float(sum(abs(mp.mpf(float(a)) * mp.mpf(float(b))) for a, b in zip(c.grad, v)))
        assert abs(float(mp.mpf(float(c.grad @ v)) - g_mp)) <= 2 * _tol(spec) * gs
        hs = float(np.abs(v) @ (np.abs(np.diag(c.d)) + np.outer(np.abs(c.p), np.abs(c.p))) @ np.abs(w))
        assert abs(float(mp.mpf(float(v @ H @ w)) - h_mp)) <= 4 * _tol(spec) * hs


@pytest.mark.parametrize("spec,s,z", _points(G.SHAPES + G.BIG_SHAPES[:2], 7))
def test_gradient_primal_by_its_two_defining_conditions(spec, s, z):
    c = ipm._make_cones([spec])[0]
    g = c.gradient_primal(s)
    assert abs(s @ g + (spec.dim1 + 1)) <= 1e-9 * (spec.dim1 + 1)
    back, _ = c.dual_grad_H(-g)
    # _newton_raphson_onesided stops BEFORE taking a step smaller than sqrt(eps) |x| (coneops_nonsymmetric_common.jl:
    # 170-193), so the root it returns is off by up to sqrt(eps) = 1.5e-8 relative; grad f* carries that to s amplified
    # by up to phi / zeta <= 1 / (1 - 0.9^2) = 5.3 (random_interior_pair keeps ||w|| under 0.9 of its bound)
    assert np.abs(back + s).max() <= 5.3 * np.sqrt(np.finfo(float).eps) * np.abs(s).max()


_mixed_problem, MIXED = G.mixed_problem, G.MIXED


def test_expanded_kkt_eliminates_to_the_reduced_dense_system():
    P, A, s, z = _mixed_problem(11, MIXED)
    mu = 0.7
    cones = G.scale_cones(MIXED, s, z, mu)
    S = G.expanded_structure(P, A, MIXED)
    assert S["p"] == 2 + 3 + 3 + 2 + 3
    K = G.expanded_matrix(S, G.expanded_values(S, cones)).toarray()
    n, m = S["n"], S["m"]
    Kr = G.reduced_matrix(P, A, cones)
    # zero-cone rows make both singular on their own block only when A has no entries there; a small shift on both
    shift = np.diag(np.concatenate([np.zeros(n), -1e-3 * np.ones(m)]))
    K[:n + m, :n + m] += shift
    Kr += shift
    rng = np.random.default_rng(3)
    rhs = rng.standard_normal(n + m)
    full = np.linalg.solve(K, np.concatenate([rhs, np.zeros(S["p"])]))
    red = np.linalg.solve(Kr, rhs)
    assert np.abs(full[:n + m] - red).max() <= 1e-9 * max(1.0, np.abs(red).max())
    # the pattern: rows ascend within a column, the diagonal is last, the signs follow the maps
    for j in range(S["N"]):
        rows = S["indices"][S["indptr"][j]:S["indptr"][j + 1]]
        assert np.all(np.diff(rows) > 0) and rows[-1] == j
    assert list(S["maps"]["dsigns"][n + m:]) == [-1, 1, -1, -1, 1, -1, -1, 1, -1, 1, -1, -1, 1]


def test_basic_genpow_through_the_driver_on_the_scipy_backend():
    P, q, A, b, cones, exp = F.basic_genpow()
    r = ipm.solve(P, q, A, b, cones, G.ExpandedScipyBackend(P, A, cones))
    print(r.status, r.iterations, r.obj_val)
    assert r.status == exp["status"] == ipm.SOLVED
    assert abs(r.obj_val - exp["obj"]) <= F.ATOL


def test_genpow_with_two_alphas_and_the_power_cone_describe_the_same_set():
    P, q, A, b, cones, exp = F.basic_genpow()
    r_gen = ipm.solve(P, q, A, b, cones, G.ExpandedScipyBackend(P, A, cones))
    # the same data with PowerConeT(alpha): basic_pow states it with the two equality rows negated
    Pp, qp, Ap, bp, cones_p, exp_p = FN.basic_pow()
    assert [c.alpha for c in cones_p[:2]] == [c.alpha[0] for c in cones[:2]]
    r_pow = ipm.solve(Pp, qp, Ap, bp, cones_p, G.ExpandedScipyBackend(Pp, Ap, cones_p))
    assert r_gen.status == r_pow.status == ipm.SOLVED
    assert abs(r_gen.obj_val - r_pow.obj_val) <= F.ATOL


def test_constructor_validation_and_ragged_parameters():
    c = GenPowerConeT([0.25, 0.25, 0.5], 4)
    assert (c.dim, c.numel, c.dim1, c.dim2, c.kind) == (7, 7, 3, 4, KIND_GENPOW == 6 and 6)
    for bad in ([0.5, 0.6], [1.5, -0.5], [0.5, float("nan")], [0.0, 1.0], []):
        with pytest.raises(ValueError):
            GenPowerConeT(bad, 1)
    with pytest.raises(ValueError):
        GenPowerConeT([1.0], 0)
    n = 40
    a = np.full(n, 1.0 / n)                                # sums to 1 within eps n / 2, not exactly
    GenPowerConeT(a, 1)
    cones = [ZeroConeT(2), PowerConeT(0.3), c, NonnegativeConeT(1), GenPowerConeT([1.0], 2)]
    ptr, vals = cone_param_ptr_vals(cones)
    assert list(ptr) == [0, 0, 1, 4, 4, 5] and list(vals) == [0.3, 0.25, 0.25, 0.5, 1.0]
    assert list(cone_params(cones)) == [0.0, 0.3, 0.0, 0.0, 0.0]
    assert has_nonsymmetric(cones) and has_nonsymmetric([c]) and not has_nonsymmetric(cones[:1])
    assert ipm._make_cones([c])[0].degree == 4
