"""tests/iterate_reference.py judged on the host: its exact values against mpmath, a plain numpy restatement of
hipkkt_kkt_system_residuals within a quarter of every bound on every builder (where a quarter of the bound is less than
the rounding u |value| of the stored fp64 value itself -- a row of one or two entries: gamma_2 / 4 = u / 2 -- that
rounding is what is allowed: no fp64 result can do better), and each simulated kernel fault breaking a
bound on every builder it can occur on (the five faults that concern A, s or Hs need a row of A: the unconstrained
builder, m = 0, has none and sees the tau fault alone)."""
import mpmath
import numpy as np
import pytest

from tests import iterate_reference as ir


@pytest.mark.parametrize("name", ["edges", "n1m1", "dense_col_4097"])
def test_exact_vectors_agree_with_mpmath(name):
    pb = ir.problem(name)
    P, A = pb.parts.P.toarray(), pb.parts.A.toarray()
    rows_x = sorted({0, pb.n // 2, pb.n - 1, min(2, pb.n - 1)})
    rows_z = sorted({0, pb.m // 2, pb.m - 1})
    with mpmath.workdps(60):
        mp = lambda v: [mpmath.mpf(float(t)) for t in v]
        x, z, tau = mp(pb.x), mp(pb.z), mpmath.mpf(pb.tau)
        for i in rows_x:
            Px = mpmath.fsum(mpmath.mpf(float(P[i, j])) * x[j] for j in np.flatnonzero(P[i]))
            Atz = mpmath.fsum(mpmath.mpf(float(A[j, i])) * z[j] for j in np.flatnonzero(A[:, i]))
            want = dict(Px=Px, rx_inf=-Atz, rx=-Atz - Px - mpmath.mpf(float(pb.q[i])) * tau)
            for k, w in want.items():
                hi, lo = pb.exact[k]
                assert abs(mpmath.mpf(float(hi[i])) + mpmath.mpf(float(lo[i])) - w) <= mpmath.mpf(2) ** -95 * (abs(w) + 1), (k, i)
        for i in rows_z:
            Ax = mpmath.fsum(mpmath.mpf(float(A[i, j])) * x[j] for j in np.flatnonzero(A[i]))
            rzi = Ax + mpmath.mpf(float(pb.s[i]))
            want = dict(rz_inf=rzi, rz=rzi - mpmath.mpf(float(pb.b[i])) * tau)
            for k, w in want.items():
                hi, lo = pb.exact[k]
                assert abs(mpmath.mpf(float(hi[i])) + mpmath.mpf(float(lo[i])) - w) <= mpmath.mpf(2) ** -95 * (abs(w) + 1), (k, i)


def test_exact_norm_over_the_whole_range():
    v = np.array([3e200, -4e200, 1e-200, 0.0])
    assert abs(ir.norm_exact(None, v) / mpmath.mpf(5e200) - 1) < 1e-15
    assert ir.norm_exact(None, np.zeros(3)) == 0 and ir.norm_exact(None, np.zeros(0)) == 0
    assert abs(ir.norm_exact(np.array([2.0, 0.5]), np.array([3e-200, 16e-200])) / mpmath.mpf(1e-199) - 1) < 1e-15
    assert ir.norm_ratio(5e200, None, v[:2]) <= 1.0 and ir.norm_ratio(float("inf"), None, v) == float("inf")
    assert ir.norm_ratio(0.0, None, np.array([1e-200])) > 1.0 and ir.norm_ratio(0.0, None, np.zeros(2)) == 0.0


@pytest.mark.parametrize("name", sorted(ir.BUILDERS))
@pytest.mark.parametrize("equil", [False, True])
def test_numpy_restatement_stays_within_a_quarter_of_every_bound(name, equil):
    pb = ir.problem(name)
    eq = ir.equil_vectors(pb) if equil else None
    # (evaluated in the x87 extended format and rounded once: a one-entry row evaluated in fp64 may use half of gamma_2)
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "this test needs a long double wider than fp64"
    vec, scal = ir.restate(pb.parts, equil=eq, dtype=np.longdouble, **pb.data())
    r = ir.vector_ratios(pb, pb.data(), vec, pb.exact, pb.bounds, share=0.25)
    r.update(ir.scalar_ratios(pb.data(), vec, scal, eq, share=0.25))
    assert set(r) == set(ir.VECTORS) | set(ir.SCALARS)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


def _faults_of(pb):
    return ir.FAULTS if pb.parts.A.nnz else ("no_tau",)


@pytest.mark.parametrize("name", sorted(ir.BUILDERS))
def test_every_simulated_fault_breaks_a_bound(name):
    pb = ir.problem(name)
    stale = ir.stale_parts(pb)
    for fault in _faults_of(pb):
        vec, _ = ir.restate(pb.parts, fault=fault, A_stale=stale, **pb.data())
        r = ir.vector_ratios(pb, pb.data(), vec, pb.exact, pb.bounds)
        assert max(r.values()) > 1.0, (fault, r)


def test_a_wrong_scalar_is_seen_apart_from_the_vectors():
    """the scalars are judged against the vectors they were formed from: a correct reduction of a faulty vector passes,
    a reduction that lost its last element fails"""
    pb = ir.problem("edges")
    vec, scal = ir.restate(pb.parts, fault="no_s", **pb.data())
    assert max(ir.scalar_ratios(pb.data(), vec, scal).values()) <= 1.0
    good_vec, good = ir.restate(pb.parts, **pb.data())
    for k in range(12):
        bad = good.copy()
        if k < 4:
            a, c = [(pb.q, pb.x), (pb.b, pb.z), (pb.s, pb.z), (pb.x, good_vec["Px"])][k]
            bad[k] = a[:-1] @ c[:-1]
            if a[-1] * c[-1] == 0.0:
                continue                              # (x . Px: the last variable has no P entry)
        else:
            v = [pb.x, pb.z, pb.s, good_vec["rx_inf"], good_vec["Px"], good_vec["rz_inf"], good_vec["rz"], good_vec["rx"]][k - 4]
            bad[k] = np.linalg.norm(v[:-1])
            if v[-1] == 0.0:
                continue                              # (the variable nothing touches: Px and rx_inf end in an exact 0)
        r = ir.scalar_ratios(pb.data(), good_vec, bad)
        assert r[ir.SCALARS[k]] > 1.0, (ir.SCALARS[k], r)
