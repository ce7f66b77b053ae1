"""tests/system_reference.py against itself on the CPU: the numpy restatement of kkt_solve! meets every derived bound at a
quarter on every builder, every simulated kernel fault pushes a defect past its bound, the oracle's refined solves stay
inside bound (1), and the tau-row identity is exact."""
from fractions import Fraction

import numpy as np
import pytest

from tests import system_reference as S

CASES = [(n, s) for n in S.BUILDERS for s in S.SCALES]
PREV_SEED = S.ITERATE_SEED + 10                     # the (s, z) of the iteration before (the stale faults)


@pytest.mark.parametrize("name,scale", CASES)
def test_restatement_meets_every_bound_at_a_quarter(name, scale):
    pb, it, rhs, view, _ = S.host_view(name, scale)
    for affine in (True, False):
        r = S.step_ratios(view, it, rhs, S.restate_step(view, it, rhs, affine), affine, share=0.25)
        print(name, scale, "affine" if affine else "combined", {k: f"{v:.3g}" for k, v in r.items()})
        assert max(r.values()) <= 1.0, (affine, r)


@pytest.mark.parametrize("name,scale", CASES)
def test_oracle_refined_solves_stay_inside_bound_1(name, scale):
    """bound (1) is a property of the inputs: a step built on the oracle's own refined solves (reference's stopping rule,
    default tolerances) stays inside it.  A builder on which it does not was replaced (see iterate())."""
    pb, it, rhs, _, o = S.host_view(name, scale)
    ov = S.oracle_view(pb, o)
    for affine in (True, False):
        r = S.step_ratios(ov, it, rhs, S.restate_step(ov, it, rhs, affine), affine, which=(1,))
        assert r[1] <= 1.0, (affine, r)


# every (builder, fault) pair that does not apply, and why: nothing else may be waved through
NOT_APPLICABLE = {(n, f) for n in ("lp1", "lp33", "lp257") for f in ("drop_P_entry", "no_2", "drop_xm_row")}     # P is empty
NOT_APPLICABLE |= {("m0", f) for f in ("flip_rhs_z", "stale_cache", "stale_x2_tail")}   # no z block; K independent of (s, z)
NOT_APPLICABLE |= {(n, "psd_offdiag") for n in S.BUILDERS if n not in ("mixed", "psd", "interleaved")}    # no PSD cone


def test_the_pairs_that_do_not_apply_are_exactly_the_listed_ones():
    got = {(n, f) for n in S.BUILDERS for f in S.STEP_FAULTS if not S.fault_applies(S.problem(n), f)}
    assert got == NOT_APPLICABLE


@pytest.mark.parametrize("name", list(S.BUILDERS))
def test_every_simulated_fault_is_caught(name):
    for scale in S.SCALES:
        pb, it, rhs, view, _ = S.host_view(name, scale)
        prev = S.host_view(name, scale, PREV_SEED)[3]
        for affine in (True, False):
            for fault in S.STEP_FAULTS:
                if not S.fault_applies(pb, fault, affine):
                    assert (name, fault) in NOT_APPLICABLE or (fault == "psd_offdiag" and affine)
                    continue
                step = S.restate_step(view, it, rhs, affine, fault=fault, prev=prev)
                order = (3, 2, 1, 4)
                r = S.step_ratios(view, it, rhs, step, affine, which=order, stop_above=1.0)
                assert max(r.values()) > 1.0, (scale, affine, fault, r)


def test_tau_row_identity_is_exact_for_vectors_that_solve_nothing():
    """N - dtau D, formed from arbitrary (x1, z1, x2, z2), equals defect (2) of (x1 + dtau x2, z1 + dtau z2, dtau) as
    rationals: small integers, tau a power of two and dtau = 3/8, so that every fp64 operation involved is exact."""
    pb = S.problem("mixed")
    rng = np.random.default_rng(5)
    n, m = pb.n, pb.m
    I = lambda k: rng.integers(-9, 10, k).astype(np.float64)
    x1, x2, z1, z2, x, q, b = I(n), I(n), I(m), I(m), I(n), I(n), I(m)
    P = pb.Pfull.copy()
    P.data = np.round(P.data * 8.0)
    it, rhs = S.Iterate(), S.Rhs()
    it.x, it.tau, it.kappa = x, 0.5, 3.0
    rhs.tau, rhs.kappa = 5.0, -7.0
    dtau = 0.375
    Pd = P.toarray()
    F = lambda v: Fraction(float(v))
    dot = lambda a, c: sum((F(u) * F(v) for u, v in zip(a, c)), Fraction(0))
    xi = [F(v) / F(it.tau) for v in x]
    xm = [a - F(c) for a, c in zip(xi, x2)]
    Pv = lambda v: [dot(row, v) for row in Pd]
    N = F(rhs.tau) - F(rhs.kappa) / F(it.tau) + dot(q, x1) + dot(b, z1) + 2 * sum(a * c for a, c in zip(xi, Pv(x1)))
    D = F(it.kappa) / F(it.tau) - dot(q, x2) - dot(b, z2) + sum(a * c for a, c in zip(xm, Pv(xm))) - dot(x2, Pv(x2))
    fake = S._WithP(pb, P)
    fake.q, fake.b = q, b
    step = (x1 + dtau * x2, z1 + dtau * z2, None, dtau, 0.0)
    assert S.defect2_fraction(fake, it, rhs, step) == N - F(dtau) * D


@pytest.mark.parametrize("name", ["lp1", "lp33", "lp257", "n1", "n33", "n257", "large"])
def test_initial_point_restatement_and_its_faults(name):
    pb, _, _, view, _ = S.host_view(name, "unit")
    assert S.initial_point_mismatches(pb, view.solve, *S.restate_initial_point(pb, view.solve)) == 0
    for fault in S.INIT_FAULTS:
        if S.fault_applies(pb, fault):
            assert S.initial_point_mismatches(pb, view.solve, *S.restate_initial_point(pb, view.solve, fault)) > 0, fault
        else:
            assert pb.P.nnz > 0
