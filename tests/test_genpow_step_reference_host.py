"""tests/genpow_step_reference.py on the CPU: the committed numpy class ipm._GenPow against the mpmath reference at
exactly the points tests/test_gpu_genpow_step_ops.py uses (this is where BOUND_C was measured: run with -s for the
ratios), the conjugate gradient's verification, and the step-length cases against the reference alone."""
import math

import numpy as np
import pytest

from cuclarabel_amd import ipm
from tests import genpow_step_reference as gs

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |numpy - mpmath| in units of the bound with C = 1:", {k: round(v, 3) for k, v in sorted(WORST.items())},
          "recorded:", gs.NUMPY_WORST, "C:", gs.BOUND_C)


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), float(r))


def test_recorded_constants():
    for k, w in gs.NUMPY_WORST.items():
        c = gs.BOUND_C[k]
        assert c >= 1.0 and c == 2.0 ** round(math.log2(c)) and w <= c < max(2.0 * w, 1.0 + 1e-12), (k, w, c)


@pytest.mark.parametrize("name", gs.LISTS)
def test_unit_start_is_the_class(name):
    for c in gs.Case(name).cones:
        if gs.is_gp(c):
            s, z = ipm._make_cones([c])[0].unit_initialization()
            assert s.tobytes() == gs.unit_start(c).tobytes() == z.tobytes()


@pytest.mark.parametrize("name", gs.LISTS)
def test_numpy_barrier_within_C(name):
    """ipm._GenPow.compute_barrier per cone; gp_barrier_term verifies g(s) on the way (it asserts)"""
    case = gs.Case(name)
    for alpha in gs.BARRIER_ALPHAS:
        got = gs.barrier_numpy(case.cones, case.z, case.s, case.dz, case.ds, alpha)
        zp, sp_ = case.z + alpha * case.dz, case.s + alpha * case.ds
        for (c, o), i in zip(case.gp(), [i for i, c in enumerate(case.cones) if gs.is_gp(c)]):
            term = gs.gp_barrier_term(c, zp[o:o + c.numel], sp_[o:o + c.numel])
            assert math.isfinite(term[0]), "BARRIER_ALPHAS must stay interior"
            err = abs(got[i] - term[0])
            _note("bar_gp", err / (gs.U * term[1] + gs.ns.gamma(c.numel) * term[2]))       # in units of the bound with C = 1
            assert err <= gs.gp_term_bound(c, term), (name, alpha, got[i], term)
        total, bound = gs.barrier_reference(case.cones, case.z, case.s, case.dz, case.ds, alpha)
        assert math.isfinite(total) and abs(math.fsum(got) - total) <= bound


def test_closed_form_branch_and_outside():
    case = gs.Case("five")
    c, o = case.gp()[2]
    s, z = case.s[o:o + c.numel].copy(), case.z[o:o + c.numel].copy()
    s[c.dim1:] = 0.0                                                     # ||s[dim1:]|| = 0: the closed-form branch
    term = gs.gp_barrier_term(c, z, s)
    got = ipm._make_cones([c])[0].compute_barrier(z, s, 0 * z, 0 * s, 0.0)
    assert abs(got - term[0]) <= gs.gp_term_bound(c, term)
    phi, nw, _ = gs._phi_norm(c, z, True)
    z[c.dim1:] *= float((1.0001 * phi / nw) ** 0.5)                      # ||w|| just outside
    assert gs.gp_barrier_term(c, z, s)[0] == math.inf


@pytest.mark.parametrize("name", [n for n in gs.LISTS if sum(c.numel for c in gs.Case(n).cones if gs.is_gp(c)) <= 40])
def test_numpy_combined_ds_within_C(name):
    case = gs.Case(name)
    for c, o in case.gp():
        r = slice(o, o + c.numel)
        for sigma_mu in (0.3, 0.0):
            val, mag = gs.ds_rows(c, case.s[r], case.z[r], sigma_mu)
            got = gs.ds_numpy(c, case.s[r], case.z[r], case.mu, sigma_mu)
            ratio = np.abs(got - val) / (gs.U * mag)
            _note("ds_gp", ratio.max())
            assert np.all(ratio <= gs.BOUND_C["ds_gp"]), (name, ratio)


def test_step_cases_on_the_reference_alone():
    """the sequential rule equals the independent form; the binding cases land where they were placed; few exclusions"""
    cases = gs.step_cases()
    a0 = 1.0 - gs.SQRT_EPS
    for (name, kind), (case, excluded) in cases.items():
        seq = gs.step_length_sequential(case.cones, case.z, case.s, case.dz, case.ds)
        if excluded:
            continue
        assert seq == gs.step_length_independent(case.cones, case.z, case.s, case.dz, case.ds), (name, kind)
        if kind == "free":
            assert seq == a0
        elif kind == "giveup":
            assert seq == 0.0
        else:
            j = 1 if kind == "coord" else int(kind[-1])
            want = a0
            for _ in range(j + 1):
                want *= gs.BACKTRACK_STEP
            assert seq == want, (name, kind, seq, want)
    nex = sum(1 for _, ex in cases.values() if ex)
    assert nex <= 0.05 * len(cases), f"{nex} of {len(cases)} step-length cases excluded"
