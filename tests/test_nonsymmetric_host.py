"""Exponential and power cones on the host (cuclarabel_amd.ipm._Exp / _Pow) against an extended-precision oracle
that is independent of the closed forms (tests/nonsymmetric_reference.py), the secant identities of the primal-dual
scaling, its central-path fall-back, and the reference's two known answers end to end.

Bounds, none taken from what the code gives:
  grad f*, H*      the closed forms subtract terms of like size once (r = z2 - z1 - z1 log(-z3/z1) for the exponential
                   cone, psi = phi - z3^2 for the power cone) and H* divides by that difference squared: with
                   kappa = (sum of |terms|) / |difference| the forward error of a few dozen float64 operations is
                   bounded by 1e3 eps kappa^2.
  g(s)             the power cone's Newton iteration stops BEFORE applying a step smaller than sqrt(eps) |x|
                   (coneops_nonsymmetric_common.jl:185-189), so g3 is off by at most that step; g1, g2 follow from g3
                   without cancellation (g3 s3 > 0).  Twice that, 2 sqrt(eps), for both cones.
  Hs               inherits g(s)'s 2 sqrt(eps) and divides by <ds,dz> = 3 mu de1 and by de2, both differences:
                   amp = 1 / min(1, |de1|) / min(1, |de2| / (zt' H zt)); bound 16 * 2 sqrt(eps) * amp (16: the terms summed).
  secant           Hs z = s and Hs zt = st hold exactly for ANY zt with <s,zt> = -3, which the closed forms give by
                   construction; what is left is rounding through the same divisions: 1e4 eps kappa^2 amp.
"""
import numpy as np
import pytest

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import ExponentialConeT, PowerConeT
from tests import nonsymmetric_reference as R
from tests.golden import nonsymmetric_fixtures as F

EPS = np.finfo(float).eps


def _kappa(spec, z):
    if isinstance(spec, ExponentialConeT):
        l = np.log(-z[2] / z[0])
        return (abs(z[0] * l) + abs(z[0]) + abs(z[1])) / abs(-z[0] * l - z[0] + z[1])
    a = spec.alpha
    phi = (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)
    return (phi + z[2] ** 2) / (phi - z[2] ** 2)


def _amp(point, guards):
    st, H, zt = point
    de1, de2 = float(guards[0]), float(guards[1])
    ztHzt = float((zt.T * H * zt)[0])
    return 1.0 / min(1.0, abs(de1)) / min(1.0, abs(de2) / ztHzt)


POINTS = [pytest.param(kind, j, id=f"{kind}-{j}") for kind in ("exp", "pow") for j in range(24)]


@pytest.mark.parametrize("kind,j", POINTS)
def test_closed_forms_against_extended_precision(kind, j):
    spec, s, z = R.scaling_points(kind, 11, 24, 0)[j]
    c = ipm._make_cones([spec])[0]
    assert c.is_primal_feasible(s) and c.is_dual_feasible(z)
    assert c.update_scaling(s, z, 0.0, ipm.PRIMAL_DUAL)
    point = R.mp_point(spec, s, z)
    st, H, Hs, used_pd, guards = R.mp_scaling(spec, s, z, 0.0, ipm.PRIMAL_DUAL, point)
    k = _kappa(spec, z)
    e_grad, e_H = R.rel_err(c.grad, st), R.rel_err(c.H_dual, H)
    e_zt = R.rel_err(c.gradient_primal(s), point[2])
    print(f"kappa {k:.2e} grad {e_grad:.2e} H {e_H:.2e} g(s) {e_zt:.2e}")
    assert e_grad <= 1e3 * EPS * k * k
    assert e_H <= 1e3 * EPS * k * k
    assert e_zt <= 2 * np.sqrt(EPS)
    assert used_pd and c.used_primal_dual, "a random interior pair is far from the central path"
    amp = _amp(point, guards)
    e_Hs = R.rel_err(c.Hs, Hs)
    print(f"amp {amp:.2e} Hs {e_Hs:.2e}")
    assert e_Hs <= 16 * 2 * np.sqrt(EPS) * amp
    # dual strategy: mu H*(z) with the caller's mu
    assert c.update_scaling(s, z, 0.37, ipm.DUAL) and not c.used_primal_dual
    assert R.rel_err(c.Hs, R.mp_scaling(spec, s, z, 0.37, ipm.DUAL, point)[2]) <= 1e3 * EPS * k * k


@pytest.mark.parametrize("kind,j", POINTS)
def test_primal_dual_scaling_secant_identities(kind, j):
    spec, s, z = R.scaling_points(kind, 11, 24, 0)[j]
    c = ipm._make_cones([spec])[0]
    assert c.update_scaling(s, z, 0.0, ipm.PRIMAL_DUAL) and c.used_primal_dual
    point = R.mp_point(spec, s, z)
    guards = R.mp_scaling(spec, s, z, 0.0, ipm.PRIMAL_DUAL, point)[4]
    tol = 1e4 * EPS * _kappa(spec, z) ** 2 * _amp(point, guards)
    zt, st = c.gradient_primal(s), c.grad
    assert abs(s @ zt + 3) <= 1e3 * EPS * 3 and abs(z @ st + 3) <= 1e3 * EPS * _kappa(spec, z) * 3
    assert np.abs(c.Hs @ z - s).max() <= tol * np.abs(s).max()                  # Hs z = s
    assert np.abs(c.Hs @ (-zt) - (-st)).max() <= tol * np.abs(st).max()         # Hs z~ = s~
    np.testing.assert_array_equal(c.Hs, c.Hs.T)
    assert np.linalg.eigvalsh(c.Hs).min() > 0
    # the packed block is the upper triangle by columns, and mul_Hs is the plain product
    np.testing.assert_array_equal(c.get_Hs(), [c.Hs[0, 0], c.Hs[0, 1], c.Hs[1, 1], c.Hs[0, 2], c.Hs[1, 2], c.Hs[2, 2]])
    x = np.array([0.3, -1.1, 0.7])
    np.testing.assert_allclose(c.mul_Hs(x), c.Hs @ x, rtol=0, atol=8 * EPS * np.abs(c.Hs).max() * 1.1)


@pytest.mark.parametrize("spec", [ExponentialConeT()] + [PowerConeT(a) for a in R.POW_ALPHAS], ids=str)
def test_fallback_at_the_unit_initialisation_point(spec):
    c = ipm._make_cones([spec])[0]
    z, s = c.unit_initialization()
    np.testing.assert_array_equal(s, z)
    assert c.is_primal_feasible(s) and c.is_dual_feasible(z)
    de1 = c.scaling_guards(s, z)[0]
    assert abs(de1) <= np.sqrt(EPS), "s = z = unit point lies on the central ray"
    assert c.update_scaling(s, z, 123.0, ipm.PRIMAL_DUAL) and not c.used_primal_dual
    mu = (z[0] * s[0] + z[1] * s[1] + z[2] * s[2]) / 3    # the LOCAL mu, not the caller's, summed in the reference's order
    np.testing.assert_array_equal(c.Hs, mu * c.H_dual)


def test_higher_correction_cholesky_failure_branch():
    for spec in (ExponentialConeT(), PowerConeT(0.6)):
        c = ipm._make_cones([spec])[0]
        z, s = c.unit_initialization()
        c.update_scaling(s, z, 1.0, ipm.DUAL)
        ok = c.combined_ds_shift(np.array([0.1, 0.2, -0.1]), np.array([0.3, -0.2, 0.1]), 0.5)
        assert np.all(np.isfinite(ok)) and np.any(ok != c.grad * 0.5)
        c.H_dual = -np.eye(3)                            # not positive definite: eta = 0, shift = grad sigma mu
        np.testing.assert_array_equal(c.combined_ds_shift(np.ones(3), np.ones(3), 0.5), c.grad * 0.5)


@pytest.mark.parametrize("fixture", [F.basic_exp, F.basic_pow], ids=lambda f: f.__name__)
def test_reference_known_answers_end_to_end(fixture):
    P, q, A, b, cones, exp = fixture()
    be = R.OracleNonsymBackend(P, A, cones)
    r = ipm.solve(P, q, A, b, cones, be)
    print(r.status, r.iterations, r.obj_val, [p[3] for p in be.points])
    assert r.status == exp["status"] == ipm.SOLVED
    if exp["x"] is not None:
        assert np.linalg.norm(r.x - exp["x"]) <= F.ATOL
    assert abs(r.obj_val - exp["obj"]) <= F.ATOL


def test_entropy_generator_small_solves_and_is_seeded():
    from cuclarabel_amd import problems
    pb, pb2, pb3 = (problems.entropy_maximization(60, seed=s) for s in (5, 5, 6))
    np.testing.assert_array_equal(pb.b, pb2.b)
    assert not np.array_equal(pb.b, pb3.b)
    assert sum(isinstance(c, ExponentialConeT) for c in pb.cones) == 60 and pb.m == 5 + 180
    r = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, R.OracleNonsymBackend(pb.P, pb.A, pb.cones))
    assert r.status == ipm.SOLVED
    x = r.x[:60]
    assert abs(x.sum() - 1) < 1e-7 and x.min() > 0
    assert abs(-r.obj_val - (-(x * np.log(x)).sum())) < 1e-6      # the optimum IS the entropy of x
    assert -r.obj_val <= np.log(60) + 1e-8
