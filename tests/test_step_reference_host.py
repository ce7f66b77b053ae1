"""The extended-precision reference of tests/step_reference.py against the numpy fp64 cone classes of
cuclarabel_amd/ipm.py (which follow the reference solver operation by operation), at every shape tests/test_gpu_step_ops.py
uses.  This module FIXES THE CONSTANTS of the bounds: the worst error / bound of the fp64 classes must stay at or below
0.25 per quantity family, so that the device has a factor 4 over the reference's own fp64 evaluation.  It also shows that
the bounds have teeth (four planted mistakes exceed them tenfold) and pins every branch of the second-order step length
on exact data.  Worst ratios are printed under -s."""
import numpy as np
import pytest

from cuclarabel_amd import ipm
from tests import cone_reference as cr
from tests import step_reference as sr

WORST = cr.Worst("fp64 numpy cone classes against the extended-precision step reference")
HOST_SHARE = 0.25


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    WORST.report()


def _host(case):
    """ipm.py cone objects scaled at (s, z), and their scaling as the reference's exact input"""
    cones = ipm._make_cones(case.cones)
    w, lam, eta, psd = np.ones(case.m), np.zeros(case.m), np.ones(len(cones)), []
    for i, c in enumerate(cones):
        if isinstance(c, ipm._Zero) or c.n == 0:
            if isinstance(c, ipm._PSD):
                psd.append((np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0)))
            continue
        assert c.update_scaling(case.s[c.rng].copy(), case.z[c.rng].copy())
        if isinstance(c, ipm._PSD):
            lam[c.off:c.off + c.k] = c.lam
            psd.append((c.R, c.Rinv, c.lam))
        else:
            w[c.rng], lam[c.rng] = c.w, c.lam
            if isinstance(c, ipm._SOC):
                eta[i] = c.eta
    return cones, sr.Scaling(case.cones, w, eta, lam, psd)


def _each(cones, m, fn):
    out = np.zeros(m)
    for c in cones:
        if c.n:
            out[c.rng] = fn(c)
    return out


def _family_ratios(err, bound, fam):
    return {f: cr.ratio(err[fam == f], bound[fam == f]) for f in set(fam[fam != None]) if f != "zero"}   # noqa: E711


def _compare(case, where, sigma_mu=0.3, m_corr=0.7):
    cones, sc = _host(case)
    out = {}
    # affine ds and the combined step's ds
    aff = _each(cones, case.m, lambda c: c.affine_ds(case.s[c.rng]))
    val, bnd, fam = sr.ds_ref(sc, case.dz, case.ds, 0.0, 0.0, False)
    out.update(_family_ratios(aff - val, bnd, fam))
    comb = aff + _each(cones, case.m, lambda c: c.combined_ds_shift(case.dz[c.rng] * m_corr, case.ds[c.rng], sigma_mu))
    val, bnd, fam = sr.ds_ref(sc, case.dz, case.ds, sigma_mu, m_corr, True)
    for f, r in _family_ratios(comb - val, bnd, fam).items():
        out[f] = max(out.get(f, 0.0), r)
    assert np.all(comb[fam == "zero"] == 0.0)
    # step length, cone by cone (alpha_max = floatmax: the cone's own limit)
    for c, lim in zip(cones, sr.cone_step_limits(sc, case.dz, case.ds, case.z, case.s)):
        assert not lim.ambiguous, f"{where}: generated point within its bound of a branch switch ({lim.where})"
        if lim.family != "none":
            got = c.step_length(case.dz[c.rng], case.ds[c.rng], case.z[c.rng], case.s[c.rng], sr.FMAX)
            out[lim.family] = max(out.get(lim.family, 0.0), lim.ratio(got))
    # margins and the shift, primal and dual
    for v, primal in ((case.s - 0.5 * np.abs(case.s).max(), True), (0.7 * case.z, False), (1e3 * case.z, False)):
        ref = sr.shift_ref(case.cones, v, primal)
        assert ref["branch"] is not None, where
        mins, pos = sr.FMAX, 0.0
        for c in cones:
            a, b = c.margins(v[c.rng])
            mins, pos = min(mins, a), pos + b
        out[ref["min"].family or "margin"] = max(out.get(ref["min"].family, 0.0), ref["min"].ratio(mins))
        out["pos_margin"] = max(out.get("pos_margin", 0.0), cr.ratio(pos - ref["pos"], ref["bpos"]))
        deg = sr.degree(case.cones)
        target = max(1.0, 0.1 * pos / max(deg, 1))
        shifts = [-mins, target] if mins <= 0 else [target - mins] if mins < target else [0.0]
        got = v.copy()
        for a in shifts:
            for c in cones:
                c.unit_shift(got[c.rng], a, primal)
        out["shift"] = max(out.get("shift", 0.0), cr.ratio(got - ref["value"], ref["bound"]))
    WORST.add(out, where)
    bad = {k: r for k, r in out.items() if not r <= HOST_SHARE}
    assert not bad, f"{where}: fp64 classes use more than {HOST_SHARE} of the bound: {bad}"


@pytest.mark.parametrize("n", sr.NN_SIZES)
def test_nonnegative(n):
    _compare(sr.Case([("nn", n)], seed=n), f"nn {n}")


@pytest.mark.parametrize("n", sr.SOC_DIMS)
def test_second_order(n):
    _compare(sr.Case([("soc", n)], seed=n), f"soc {n}")
    _compare(sr.Case([("soc", n, 1e-8)], seed=100 + n), f"soc {n} delta 1e-8")


@pytest.mark.parametrize("ncones", (1, 4, 5))
def test_second_order_several(ncones):
    _compare(sr.Case([("soc", 5)] * ncones, seed=ncones), f"{ncones} x soc 5")


@pytest.mark.parametrize("k", sr.PSD_SIDES)
def test_psd(k):
    cls = cr.PSD_CLASSES[k % len(cr.PSD_CLASSES)]
    _compare(sr.Case([("psd", k, cls, k % 2 == 0)], seed=k), f"psd {k} {cls}")


@pytest.mark.parametrize("cls", cr.PSD_CLASSES)
def test_psd_classes(cls):
    _compare(sr.Case([("psd", 7, cls, True)], seed=3), f"psd 7 {cls} leaving")
    _compare(sr.Case([("psd", 8, cls, False)], seed=4), f"psd 8 {cls} staying")


def test_mixed_with_zero_and_empty_cones():
    _compare(sr.Case([("zero", 3), ("nn", 257), ("zero", 2), ("soc", 5), ("soc", 5), ("psd", 3, "interior", True),
                      ("psd", 0, "interior", True), ("zero", 1), ("nn", 1)], seed=9), "mixed")


# ---- the bounds have teeth: each planted mistake exceeds its bound at least tenfold
def _teeth_case(piece):
    case = sr.Case([piece], seed=5)
    cones, sc = _host(case)
    return case, cones[0], sc


def test_teeth_soc_tail_sign():
    case, c, sc = _teeth_case(("soc", 6))
    val, bnd, _ = sr.ds_ref(sc, case.dz, case.ds, 0.3, 1.0, True)
    wrong = c.affine_ds(case.s) + c.combined_ds_shift(case.dz, case.ds, 0.3)
    wrong[3] = -wrong[3]
    assert cr.ratio(wrong - val, bnd) >= 10.0


def test_teeth_psd_dropped_sqrt2():
    case, c, sc = _teeth_case(("psd", 7, "interior", True))
    val, bnd, _ = sr.ds_ref(sc, case.dz, case.ds, 0.3, 1.0, True)
    wrong = c.affine_ds(case.s) + c.combined_ds_shift(case.dz, case.ds, 0.3)
    wrong[1] /= np.sqrt(2.0)                             # svec slot 1 is the off-diagonal entry (0, 1)
    assert cr.ratio(wrong - val, bnd) >= 10.0


def test_teeth_rinv_for_r():
    case, c, sc = _teeth_case(("psd", 7, "interior", True))
    val, bnd, _ = sr.ds_ref(sc, case.dz, case.ds, 0.3, 1.0, True)
    c.R = c.Rinv.T.copy()                                # W dz formed with Rinv where R belongs
    wrong = c.affine_ds(case.s) + c.combined_ds_shift(case.dz, case.ds, 0.3)
    assert cr.ratio(wrong - val, bnd) >= 10.0


def test_teeth_larger_root():
    name, x, y, want = [t for t in sr.soc_exact_cases() if t[0] == "two positive roots"][0]
    lim = sr.soc_step_component(np.array(x), np.array(y))
    assert lim.ratio(want) == 0.0 and lim.ratio(3.0) >= 10.0        # 3 is the other root of that case


# ---- every branch of _step_length_soc_component, on exact data
@pytest.mark.parametrize("name,x,y,want", sr.soc_exact_cases(), ids=[t[0] for t in sr.soc_exact_cases()])
def test_soc_branch_exact(name, x, y, want):
    x, y = np.array(x), np.array(y)
    branch = []
    lim = sr.fold_min([sr.Limit(1.0), sr.soc_step_component(x, y, branch)])
    got = ipm._SOC._step(x, y, 1.0)
    assert got == want, (name, got)
    assert lim.ratio(got) <= HOST_SHARE, (name, lim.value, lim.lo, lim.hi)
    a, b, c = ipm._soc_res(y), 2 * (x[0] * y[0] - x[1:] @ y[1:]), max(0.0, ipm._soc_res(x))
    d = b * b - 4 * a * c
    if name == "d<0":
        # reachable by rounding alone (see soc_exact_cases): fp64 must take it here, the exact quadratic has d = 0
        assert d < 0 and not (a > 0 and b > 0) and lim.ambiguous
        return
    assert lim.value == want and not lim.ambiguous
    taken = "a>0,b>0" if (a > 0 and b > 0) else "d<0" if d < 0 else "a==0" if a == 0 else \
        ("c==0,a>=0" if a >= 0 else "c==0,a<0") if c == 0 else None
    if name == "clamp":
        assert taken == "a==0" and x[0] >= 0 and y[0] < 0 and -x[0] / y[0] == want      # the clamp is what binds
    elif taken is not None:
        assert taken == name == branch[0]
    else:
        assert branch[0] == name
