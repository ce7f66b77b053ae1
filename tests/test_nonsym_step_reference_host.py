"""Host checks of tests/nonsym_step_reference.py (no GPU): the committed numpy classes (ipm._Exp, ipm._Pow and the
symmetric ones) against the mpmath reference at every point the GPU test uses -- this is where the bound constants were
measured (worst ratios printed under -s) -- and the two forms of the composite step length against each other."""
import math

import numpy as np
import pytest

from cuclarabel_amd import ipm
from tests import nonsym_step_reference as ns

WORST = {}


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), float(r))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |numpy class - mpmath| / (u * magnitude):", {k: round(v, 3) for k, v in sorted(WORST.items())})


def ds_points():
    """(case, central) whose non-symmetric cones the d.s checks visit; the long lists hold POOL distinct points"""
    return [(name, central) for name in ns.LISTS for central in (False, True)]


@pytest.mark.parametrize("name,central", ds_points())
def test_numpy_ds_rows_within_the_bound(name, central):
    case = ns.Case(name, seed=1, central=central)
    for c, o in case.ns()[:ns.POOL]:
        r = slice(o, o + 3)
        val, mag = ns.ns_ds_rows(c, case.s[r], case.z[r], case.dz[r], case.ds[r], 0.0, 0.0, False)
        got = ns.ns_ds_numpy(c, case.s[r], case.z[r], case.dz[r], case.ds[r], case.mu, ipm.DUAL, 0.0, 0.0, False)
        assert got.tobytes() == val.tobytes() == case.s[r].tobytes()
        for sigma_mu, m_corr in ((0.3, 0.7), (0.0, 1.0)):
            val, mag = ns.ns_ds_rows(c, case.s[r], case.z[r], case.dz[r], case.ds[r], sigma_mu, m_corr, True)
            for strategy in (ipm.PRIMAL_DUAL, ipm.DUAL):
                got = ns.ns_ds_numpy(c, case.s[r], case.z[r], case.dz[r], case.ds[r], case.mu, strategy, sigma_mu, m_corr, True)
                ratio = np.abs(got - val) / (ns.U * mag)
                _note("ds_" + ns.fam(c), ratio.max())
                assert np.all(ratio <= ns.BOUND_C["ds_" + ns.fam(c)]), (name, o, ratio)


def test_eta_is_the_third_directional_derivative():
    """the reference's eta against a central difference of the Hessian along v (an independent route to D^3 f*[u, v])"""
    import mpmath as mp
    from tests import nonsymmetric_reference as nr
    case = ns.Case("mixed", seed=1)
    for c, o in case.ns():
        r = slice(o, o + 3)
        z, dz, ds, s = case.z[r], case.dz[r], case.ds[r], case.s[r]
        val, _ = ns.ns_ds_rows(c, s, z, dz, ds, 0.0, 1.0, True)
        eta = val - s                                          # sigma_mu = 0: d.s = s + eta
        with mp.workdps(60):
            f = nr.dual_barrier(c)
            h = mp.mpf(10) ** -15
            zp = [mp.mpf(float(a)) + h * mp.mpf(float(b)) for a, b in zip(z, dz)]
            zm = [mp.mpf(float(a)) - h * mp.mpf(float(b)) for a, b in zip(z, dz)]

            def hess(pt):                                          # (nr.mp_hess rounds its point to fp64)
                return mp.matrix([[mp.diff(f, pt, tuple((i == 0) + (j == 0) if False else int(i == k) + int(j == k) for k in range(3)))
                                   for j in range(3)] for i in range(3)])
            dH = (hess(zp) - hess(zm)) / (2 * h)
            u = nr.mp_hess(f, z) ** -1 * mp.matrix([float(t) for t in ds])
            want = -dH * u / 2
        assert np.allclose(eta, [float(t) for t in want], rtol=1e-9, atol=1e-9 * np.abs(eta).max())


@pytest.mark.parametrize("name", ns.LISTS)
def test_numpy_barrier_terms_within_the_bound(name):
    case = ns.Case(name, seed=1)
    for alpha in ns.BARRIER_ALPHAS:
        terms = ns.barrier_terms(case.cones, case.z, case.s, case.dz, case.ds, alpha)
        got = ns.barrier_numpy(case.cones, case.z, case.s, case.dz, case.ds, alpha)
        for (family, val, mag), g in zip(terms, got):
            if family == "zero":
                assert g == 0.0
            elif math.isfinite(val):
                ratio = abs(g - val) / (ns.U * mag)
                _note("bar_" + family, ratio)
                assert ratio <= ns.BOUND_C["bar_" + family], (name, family, ratio)
            else:
                assert not math.isfinite(g)
        total, bound = ns.barrier_sum(terms)
        assert math.isfinite(total), "the GPU test's points must stay interior at these alphas"
        assert abs(math.fsum(got) - total) <= bound
    # a step that leaves a cone: +inf
    dz = case.dz.copy()
    c, o = case.ns()[0]
    dz[o:o + 3] = -2.0 * case.z[o:o + 3]
    assert ns.barrier_sum(ns.barrier_terms(case.cones, case.z, case.s, dz, case.ds, 1.0))[0] == math.inf
    with np.errstate(all="ignore"):
        assert not math.isfinite(sum(ns.barrier_numpy(case.cones, case.z, case.s, dz, case.ds, 1.0)))


def test_step_length_independent_minimum_is_the_sequential_result():
    cases = ns.step_cases()
    excluded = [c for c in cases if c[4]]
    assert len(excluded) <= 0.05 * len(cases), f"{len(excluded)} of {len(cases)} generated cases excluded"
    for name, kind, seed, case, ex in cases:
        if ex:
            continue
        seq = ns.step_length_sequential(case.cones, case.z, case.s, case.dz, case.ds, **case.scal)
        ind = ns.step_length_independent(case.cones, case.z, case.s, case.dz, case.ds, **case.scal)
        assert seq == ind, (name, kind, seed, seq, ind)
        if kind == "free":
            assert seq == 1.0 - ns.SQRT_EPS
        elif kind in ("dual", "primal"):
            a, j = 1.0 - ns.SQRT_EPS, 0
            while a != seq:
                a, j = a * ns.BACKTRACK_STEP, j + 1
                assert a >= ns.ALPHA_MIN, (name, kind, seed, seq)
            assert j >= 2
        elif kind == "symmetric":
            assert seq == 0.5
        else:
            assert seq == 0.0
