"""The device cone operations between the solves on an opted-in handle with PSD cones of side 49 ... 96
(k_step_ds_psd_big, k_step_length_psd_big, k_margins_psd_big, k_barrier_psd_big of csrc/step_kernels.hip), against
tests/step_reference.py with the device's own scaling as exact input, the way tests/test_gpu_step_ops.py does it.

Sides 49 (odd: the dummy pair), 64 (32 pairs), 65 and 66 (the first sides a 256-thread workgroup could not pair), and one
combined-ds and one step-length case at the cap, 96.  Through the _ns family on [Exp, PSD(65), Pow] and the _gp family on
[GenPow, PSD(65)]: the unit start, the barrier against tests/nonsym_step_reference.py, and the other cones' rows as bits
of a twin handle without the PSD cone.  A handle that is not opted in is refused by all fourteen calls."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import NonnegativeConeT, PSDTriangleConeT, ExponentialConeT, PowerConeT, GenPowerConeT
from tests import cone_reference as cr
from tests import step_reference as sr
from tests import nonsym_step_reference as ns
from tests import genpow_step_reference as gs
from tests import test_gpu_step_ops as sym
from tests import test_gpu_genpow_step_ops as gp

pytestmark = pytest.mark.gpu

BIG_SIDES = (49, 64, 65, 66)


def _handle(dev, cones, large):
    import torch
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
    dev.torch, dev.cones = torch, list(cones)
    dev.m = sum(c.numel for c in cones)
    dev.ks = HipKKTSolver(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((dev.m, 2))), cones, large_psd=large)
    dev.system = HipKKTSystem(dev.ks)
    dev.system.init(np.zeros(2), np.zeros(dev.m))


class SymDev(sym.Dev):
    """test_gpu_step_ops.Dev over an opted-in handle"""

    def __init__(self, cones, s=None, z=None, large=True):
        _handle(self, cones, large)
        self.sc = None
        if s is not None:
            assert self.system.update(s, z)
            lam, psd = self.ks.scaling()
            w, eta = self.ks.scaling_w()
            self.sc = sr.Scaling(cones, w, eta, lam, psd)


class NsDev(gp.Dev):
    """test_gpu_genpow_step_ops.Dev (the _ns and the _gp calls) over an opted-in handle"""

    def __init__(self, cones, s=None, z=None, strategy=ipm.PRIMAL_DUAL, mu=1.0, large=True):
        _handle(self, cones, large)
        if s is not None:
            self.ks.set_nonsymmetric_scaling(strategy, mu)
            assert self.system.update(s, z)


_CASES = {}


def _case(k):
    """the case and its scaled handle at side k, shared by the tests of that side (beside a nonnegative cone, so that the
    elementwise workgroups run in front of the PSD slots)"""
    if k not in _CASES:
        case = sr.Case([("nn", 5), ("psd", k, "interior", True)], seed=k)
        _CASES[k] = (case, SymDev(case.cones, case.s, case.z))
    return _CASES[k]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _CASES.clear()


@pytest.mark.parametrize("k", BIG_SIDES)
def test_affine_and_combined_ds(k):
    case, dev = _case(k)
    sym._check_ds(dev, case, f"psd {k}")


@pytest.mark.parametrize("k", BIG_SIDES)
def test_step_length_binding_on_z_on_s_and_not_at_all(k):
    case, dev = _case(k)
    psd = slice(5, case.m)
    inside_z, inside_s = case.dz.copy(), case.ds.copy()
    inside_z[:5], inside_s[:5] = 0.0, 0.0
    inside_z[psd], inside_s[psd] = case.z[psd], case.s[psd]              # a positive definite step: no limit
    for what, dz, ds in (("z", np.r_[np.zeros(5), case.dz[psd]], inside_s), ("s", inside_z, np.r_[np.zeros(5), case.ds[psd]])):
        step = SimpleNamespace(cones=case.cones, z=case.z, s=case.s, dz=dz, ds=ds)
        got, ref = sym._check_step(dev, step, f"psd {k} binding on {what}")
        assert ref.family == "psd_step" and got < 1.0, (k, what, ref.family, got)
    assert dev.step_length(inside_z, inside_s, case.z, case.s) == 1.0    # nothing binds: exactly alpha_max


@pytest.mark.parametrize("k", BIG_SIDES)
def test_margins_and_the_three_branches_of_the_shift(k):
    case, dev = _case(k)
    inside = np.abs(case.z) + 0.0
    inside[sr.unit_rows(case.cones)[0]] += 50.0
    seen = sym._check_shift(dev, case, f"psd {k}", ((case.s - 2.0 * np.abs(case.s).max(), True, "outside"),
                                                    (0.01 * case.z, False, "small"), (1e4 * inside, True, "good")))
    assert seen == {"outside", "small", "good"}


def test_side_96_combined_ds_and_step_length():
    case = sr.Case([("psd", 96, "interior", True)], seed=96)
    dev = SymDev(case.cones, case.s, case.z)
    got = dev.combined_ds(case.dz, case.ds, sym.SIGMA_MU, sym.M_CORR)
    val, bnd, fam = sr.ds_ref(dev.sc, case.dz, case.ds, sym.SIGMA_MU, sym.M_CORR, True)
    sym._within(sym._family_ratios(got - val, bnd, fam), "psd 96 combined ds")
    got, ref = sym._check_step(dev, case, "psd 96")
    assert ref.family == "psd_step" and got < 1.0


def test_small_and_big_psd_cones_on_one_handle():
    """both PSD classes at once: the big class's slots sit behind the small class's in every partials array
    (partial + ge + nsoc + npsd), with elementwise workgroups and a second-order cone in front of both"""
    pieces = [("nn", 5), ("psd", 8, "interior", True), ("soc", 6), ("psd", 49, "interior", True), ("psd", 3, "interior", True),
              ("psd", 65, "interior", False)]
    case = sr.Case(pieces, seed=7)
    dev = SymDev(case.cones, case.s, case.z)
    sym._check_ds(dev, case, "small + big")
    got, ref = sym._check_step(dev, case, "small + big")
    assert got < 1.0
    # each class binding alone: the other class's cones step along an interior direction
    off = np.cumsum([0] + [c.numel for c in case.cones])
    for binding in (1, 3):                                               # PSD(8), PSD(49)
        dz, ds = case.z.copy(), case.s.copy()
        r = slice(off[binding], off[binding + 1])
        dz[r], ds[r] = case.dz[r], case.ds[r]
        step = SimpleNamespace(cones=case.cones, z=case.z, s=case.s, dz=dz, ds=ds)
        got, ref = sym._check_step(dev, step, f"small + big, cone {binding} binding")
        assert ref.family == "psd_step" and got < 1.0
    sym._check_shift(dev, case, "small + big", ((case.s - 2.0 * np.abs(case.s).max(), True, "outside"),))


def test_barrier_slots_with_both_psd_classes_and_the_lane_per_cone_part():
    """[Exp, PSD(3), PSD(49), Pow]: small-class slots, lane-per-cone workgroups' slots, then the big class's"""
    cones = [ExponentialConeT(), PSDTriangleConeT(3), PSDTriangleConeT(49), PowerConeT(0.4)]
    off, s, z, mu, dz, ds = _ns_point(cones, 2)
    dev = NsDev(cones, s, z, ipm.DUAL, mu)
    for alpha in ns.BARRIER_ALPHAS:
        bar, _dot = dev.barrier(z, s, dz, ds, alpha)
        total, bound = ns.barrier_sum(ns.barrier_terms(cones, z, s, dz, ds, alpha), ns.DEVICE_FACTOR)
        assert math.isfinite(total) and abs(bar - total) <= bound, (alpha, bar, total, bound)
    # a step that leaves only the big cone: +inf from its slot alone
    bad = np.zeros_like(z)
    bad[off[2]:off[2] + cones[2].numel] = -2.0 * z[off[2]:off[2] + cones[2].numel]
    bar, _dot = dev.barrier(z, s, bad, np.zeros_like(s), 1.0)
    assert bar == math.inf


# ---- through the _ns and the _gp families ---------------------------------------------------------------------------------
def _ns_point(cones, seed):
    """an interior (s, z) with a short step, cone by cone"""
    from tests import nonsymmetric_reference as nr
    from tests import genpow_reference as gr
    rng = np.random.default_rng([seed, 65])
    off = ns.offsets(cones)
    m = sum(c.numel for c in cones)
    s, z = np.zeros(m), np.zeros(m)
    for c, o in zip(cones, off):
        r = slice(o, o + c.numel)
        if isinstance(c, PSDTriangleConeT):
            s[r], z[r] = cr.psd_pair(rng, c.dim, "interior")
        else:
            s[r], z[r] = (gr if gs.is_gp(c) else nr).random_interior_pair(c, rng)
    mu = float(s @ z) / sum(ipm._make_cones([c])[0].degree for c in cones)
    return off, s, z, mu, 0.01 * rng.normal(size=m) * np.abs(z).max(), 0.01 * rng.normal(size=m) * np.abs(s).max()


@pytest.mark.parametrize("family", ["ns", "gp"])
def test_ns_and_gp_families_beside_a_psd_65(family):
    cones = [ExponentialConeT(), PSDTriangleConeT(65), PowerConeT(0.7)] if family == "ns" else \
        [GenPowerConeT((0.3, 0.7), 2), PSDTriangleConeT(65)]
    off, s, z, mu, dz, ds = _ns_point(cones, 1)
    rows = np.ones(len(s), bool)
    rows[off[1]:off[1] + cones[1].numel] = False                         # the rows of the other cones
    others = [c for c in cones if not isinstance(c, PSDTriangleConeT)]
    dev = NsDev(cones, s, z, ipm.DUAL, mu)
    twin = NsDev(others, s[rows], z[rows], ipm.DUAL, mu, large=False)
    call = (lambda d, name: getattr(d, name if family == "ns" else
                                    {"unit_initialization": "unit_initialization_gp", "affine_ds_ns": "affine_ds_gp",
                                     "combined_ds_ns": "combined_ds_gp", "step_length_ns": "step_length_gp",
                                     "barrier": "barrier_gp"}[name]))
    # the unit start: svec(I) on the PSD rows, the twin's bits elsewhere
    us, uz = call(dev, "unit_initialization")()
    ts, tz = call(twin, "unit_initialization")()
    eye = cr.svec(np.eye(65))
    assert us[~rows].tobytes() == eye.tobytes() and uz[~rows].tobytes() == eye.tobytes()
    assert us[rows].tobytes() == ts.tobytes() and uz[rows].tobytes() == tz.tobytes()
    # ds: the other cones' rows are the twin's bits; the PSD rows are those of the symmetric reference
    got = call(dev, "affine_ds_ns")(s)
    assert got[rows].tobytes() == call(twin, "affine_ds_ns")(s[rows]).tobytes()
    got = call(dev, "combined_ds_ns")(dz, ds, s, z, 0.3, 0.7)
    assert got[rows].tobytes() == call(twin, "combined_ds_ns")(dz[rows], ds[rows], s[rows], z[rows], 0.3, 0.7).tobytes()
    lam, psd = dev.ks.scaling()
    w, eta = dev.ks.scaling_w()
    p = slice(off[1], off[1] + cones[1].numel)
    sc = sr.Scaling([cones[1]], w[p], eta[1:2], lam[p], psd)
    val, bnd, fam = sr.ds_ref(sc, dz[p], ds[p], 0.3, 0.7, True)
    sym._within(sym._family_ratios(got[p] - val, bnd, fam), f"{family}: psd 65 combined ds")
    # the barrier against the reference at its bound
    for alpha in ns.BARRIER_ALPHAS:
        bar, _dot = call(dev, "barrier")(z, s, dz, ds, alpha)
        total, bound = gs.barrier_reference(cones, z, s, dz, ds, alpha, gs.DEVICE_FACTOR) if family == "gp" else \
            ns.barrier_sum(ns.barrier_terms(cones, z, s, dz, ds, alpha), ns.DEVICE_FACTOR)
        assert math.isfinite(total)
        assert abs(bar - total) <= bound, (family, alpha, bar, total, bound)
    # a short step: the common start 1 - sqrt(eps) survives every cone
    assert call(dev, "step_length_ns")(1e-3 * z, 1e-3 * s, z, s) == 1.0 - ns.SQRT_EPS


# ---- a handle that is not opted in ------------------------------------------------------------------------------------------
def test_a_handle_that_is_not_enabled_is_refused_by_all_fourteen_calls():
    import torch
    from cuclarabel_amd import _lib
    from tests.test_gpu_step_entry_matrix import FAMILY
    L = _lib.lib()
    for cones in ([NonnegativeConeT(2), PSDTriangleConeT(49)], [NonnegativeConeT(2), PSDTriangleConeT(97)]):
        for large in ((False,) if cones[1].dim == 49 else (False, True)):
            dev = NsDev(cones, large=large)
            h, m = dev.ks._h, dev.m
            o = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
            o2 = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
            a = torch.ones(m, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            O, O2, A = o.data_ptr(), o2.data_ptr(), a.data_ptr()
            a1, a2 = np.full(1, 7.0), np.full(2, 7.0)
            calls = {
                "hipkkt_kkt_system_affine_ds": lambda f: f(h, O),
                "hipkkt_kkt_system_combined_ds": lambda f: f(h, O, A, A, 0.3, 0.7),
                "hipkkt_kkt_system_step_length": lambda f: f(h, A, A, A, A, 1.0, 1.0, 1.0, 1.0, _lib.ptr(a1)),
                "hipkkt_kkt_system_shift_to_interior": lambda f: f(h, O, 1, _lib.ptr(a2)),
            }
            for sfx in ("_ns", "_gp"):
                tail = "" if sfx == "_ns" else sfx
                calls["hipkkt_kkt_system_unit_initialization" + tail] = lambda f: f(h, O, O2)
                calls["hipkkt_kkt_system_affine_ds" + sfx] = lambda f: f(h, O, A)
                calls["hipkkt_kkt_system_combined_ds" + sfx] = lambda f: f(h, O, A, A, A, A, 0.3, 0.7)
                calls["hipkkt_kkt_system_step_length" + sfx] = lambda f: f(h, A, A, A, A, 1.0, 1.0, 1.0, 1.0, gs.BACKTRACK_STEP,
                                                                           gs.ALPHA_MIN, _lib.ptr(a1))
                calls["hipkkt_kkt_system_barrier" + tail] = lambda f: f(h, A, A, A, A, 0.01, _lib.ptr(a2))
            assert sorted(calls) == sorted(FAMILY)
            want = "side > 96" if large else "side > 48"
            for name, call in calls.items():
                assert call(getattr(L, name)) == -1, name                # HIPKKT_ERR_ARG
                assert want in L.hipkkt_last_error().decode(), (name, L.hipkkt_last_error())
            dev.ks.synchronize()
            assert np.all(o.cpu().numpy() == 7.0) and np.all(o2.cpu().numpy() == 7.0) and a1[0] == 7.0 and \
                np.all(a2 == 7.0), "a refused call wrote something"
