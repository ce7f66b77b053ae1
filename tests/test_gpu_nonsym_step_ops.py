"""The device cone operations between the solves on cone lists that hold exponential and power cones
(hipkkt_kkt_system_unit_initialization / _affine_ds_ns / _combined_ds_ns / _step_length_ns / _barrier:
csrc/step_kernels.hip) against tests/nonsym_step_reference.py.

Cone lists: one exponential cone; one power cone; every symmetric kind with non-symmetric cones at odd offsets in
between; 255, 256 and 257 exponential cones behind a nonnegative row (the workgroup boundary of the lane-per-cone kernels
and more than one partial for the finishing kernels).  Points: random interior pairs and central-path pairs, scaled
under both strategies.  The non-symmetric rows are held to DEVICE_FACTOR times the bound the numpy classes were measured
against; the symmetric rows must equal, bit for bit, what the symmetric entry points give on a twin handle with only
those cones; the step length must equal the host's sequential restatement as a double.  Every operation is called twice
and must repeat bit for bit."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT, PowerConeT,
                                  GenPowerConeT)
from tests import iterate_reference as ir
from tests import nonsym_step_reference as ns

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst device error / (DEVICE_FACTOR * bound):", {k: round(v, 4) for k, v in sorted(WORST.items())})


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), float(r))


class Dev:
    """a level-C handle over a cone list (P = I_2, A = ones(m, 2)), scaled at (s, z) under `strategy` unless s is None"""

    def __init__(self, cones, s=None, z=None, strategy=ipm.PRIMAL_DUAL, mu=1.0):
        import torch
        from cuclarabel_amd import _lib
        from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
        assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
        self.torch, self.cones = torch, list(cones)
        self.m = sum(c.numel for c in cones)
        self.ks = HipKKTSolver(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((self.m, 2))), cones)
        self.system = HipKKTSystem(self.ks)
        self.system.init(np.zeros(2), np.zeros(self.m))
        if s is not None:
            self.ks.set_nonsymmetric_scaling(strategy, mu)
            assert self.system.update(s, z)

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
        self.torch.cuda.synchronize()
        return t

    def down(self, t):
        self.ks.synchronize()
        return t.cpu().numpy()

    def out(self):
        t = self.torch.full((max(self.m, 1),), float("nan"), dtype=self.torch.float64, device="cuda")
        self.torch.cuda.synchronize()
        return t

    @staticmethod
    def twice(fn):
        a, b = np.asarray(fn()), np.asarray(fn())
        assert a.tobytes() == b.tobytes(), "the same call on the same data gave other bits"
        return a

    def unchanged(self, pairs):
        for t, a in pairs:
            assert self.down(t).tobytes() == np.ascontiguousarray(a, dtype=np.float64).tobytes(), "an input was modified"

    def unit_initialization(self):
        def run():
            s, z = self.out(), self.out()
            assert self.system.unit_initialization_dev(s.data_ptr(), z.data_ptr())
            return np.r_[self.down(s)[:self.m], self.down(z)[:self.m]]
        r = self.twice(run)
        return r[:self.m], r[self.m:]

    def affine_ds_ns(self, s):
        ts = self.up(s)

        def run():
            o = self.out()
            assert self.system.affine_ds_ns_dev(o.data_ptr(), ts.data_ptr())
            return self.down(o)[:self.m]
        got = self.twice(run)
        self.unchanged([(ts, s)])
        return got

    def combined_ds_ns(self, dz, ds, s, z, sigma_mu, m_corr):
        t = [self.up(v) for v in (dz, ds, s, z)]

        def run():
            o = self.out()
            assert self.system.combined_ds_ns_dev(o.data_ptr(), *[v.data_ptr() for v in t], sigma_mu, m_corr)
            return self.down(o)[:self.m]
        got = self.twice(run)
        self.unchanged(zip(t, (dz, ds, s, z)))
        return got

    def sym_ds(self, dz, ds, sigma_mu, m_corr, combined):
        """the existing symmetric entry points (a twin handle)"""
        o = self.out()
        if combined:
            tz, ts = self.up(dz), self.up(ds)
            assert self.system.combined_ds_dev(o.data_ptr(), tz.data_ptr(), ts.data_ptr(), sigma_mu, m_corr)
        else:
            assert self.system.affine_ds_dev(o.data_ptr())
        return self.down(o)[:self.m]

    def step_length_ns(self, dz, ds, z, s, step=ns.BACKTRACK_STEP, amin=ns.ALPHA_MIN, **scal):
        t = [self.up(v) for v in (dz, ds, z, s)]
        got = float(self.twice(lambda: self.system.step_length_ns_dev(
            *[v.data_ptr() for v in t], scal.get("dtau", 1.0), scal.get("dkappa", 1.0), scal.get("tau", 1.0),
            scal.get("kappa", 1.0), step, amin)))
        self.unchanged(zip(t, (dz, ds, z, s)))
        return got

    def barrier(self, z, s, dz, ds, alpha):
        t = [self.up(v) for v in (z, s, dz, ds)]
        got = self.twice(lambda: np.array(self.system.barrier_dev(*[v.data_ptr() for v in t], alpha)))
        self.unchanged(zip(t, (z, s, dz, ds)))
        return float(got[0]), float(got[1])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ns.LISTS)
def test_unit_initialization(name):
    """exact equality with the host classes; needs no scaling"""
    cones = ns._list(name)
    dev = Dev(cones)
    s, z = dev.unit_initialization()
    want = [c.unit_initialization() for c in ipm._make_cones(cones)]
    assert z.tobytes() == np.concatenate([w[0] for w in want]).tobytes()
    assert s.tobytes() == np.concatenate([w[1] for w in want]).tobytes()


def test_unit_initialization_every_power_alpha_and_larger_symmetric_cones():
    cones = [PowerConeT(a) for a in (0.1, 0.5, 0.6, 0.9, 1.0 / 3.0)] + [SecondOrderConeT(5), PSDTriangleConeT(4), ZeroConeT(2),
                                                                        NonnegativeConeT(300), ExponentialConeT()]
    s, z = Dev(cones).unit_initialization()
    want = [c.unit_initialization() for c in ipm._make_cones(cones)]
    assert z.tobytes() == np.concatenate([w[0] for w in want]).tobytes()
    assert s.tobytes() == np.concatenate([w[1] for w in want]).tobytes()


@pytest.mark.parametrize("strategy", (ipm.PRIMAL_DUAL, ipm.DUAL))
@pytest.mark.parametrize("central", (False, True))
@pytest.mark.parametrize("name", ns.LISTS)
def test_affine_and_combined_ds(name, central, strategy):
    case = ns.Case(name, seed=1, central=central)
    dev = Dev(case.cones, case.s, case.z, strategy, case.mu)
    sym_cones, sym = case.twin()
    twin = Dev(sym_cones, case.s[sym], case.z[sym]) if sym_cones else None
    zero = np.zeros(case.m, bool)
    for c, o in zip(case.cones, case.off):
        if isinstance(c, ZeroConeT):
            zero[o:o + c.numel] = True

    got = dev.affine_ds_ns(case.s)
    assert got[~sym].tobytes() == case.s[~sym].tobytes(), "affine_ds_ns: the non-symmetric rows are a copy of s"
    if twin:
        assert got[sym].tobytes() == twin.sym_ds(None, None, 0.0, 0.0, False).tobytes(), "affine_ds_ns: symmetric rows"
    assert np.all(got[zero] == 0.0)

    for sigma_mu, m_corr in ((0.3, 0.7), (0.0, 1.0)):
        got = dev.combined_ds_ns(case.dz, case.ds, case.s, case.z, sigma_mu, m_corr)
        if twin:
            want = twin.sym_ds(case.dz[sym], case.ds[sym], sigma_mu, m_corr, True)
            assert got[sym].tobytes() == want.tobytes(), "combined_ds_ns: symmetric rows differ from hipkkt_kkt_system_combined_ds"
        assert np.all(got[zero] == 0.0)
        for c, o in case.ns():
            r = slice(o, o + 3)
            val, mag = ns.ns_ds_rows(c, case.s[r], case.z[r], case.dz[r], case.ds[r], sigma_mu, m_corr, True)
            ratio = np.abs(got[r] - val) / (ns.DEVICE_FACTOR * ns.BOUND_C["ds_" + ns.fam(c)] * ns.U * mag)
            _note("ds_" + ns.fam(c), ratio.max())
            assert np.all(ratio <= 1.0), (name, o, sigma_mu, m_corr, ratio)


_STEP_PARAMS = [(name, kind, seed) for name in ns.LISTS for kind in ns.STEP_KINDS
                for seed in ((1, 2, 3) if name in ("exp", "pow", "mixed") else (1,))]
_STEP_CASES = {}


def _step_case(name, kind, seed):
    if not _STEP_CASES:
        for nm, kd, sd, case, excluded in ns.step_cases():
            _STEP_CASES[(nm, kd, sd)] = (case, excluded)
    return _STEP_CASES[(name, kind, seed)]


@pytest.mark.parametrize("name,kind,seed", _STEP_PARAMS)
def test_step_length(name, kind, seed):
    """equal as doubles to the host's sequential composite rule: nothing binds / the dual side of one cone binds after
    j >= 2 backtracks / the primal side does / a symmetric limit (or tau) sets the start below 1 - sqrt(eps) / a direction
    that leaves the cone at once.  An excluded case (a feasibility test within its evaluation bound of the boundary) must
    still give a value the search visits."""
    case, excluded = _step_case(name, kind, seed)
    dev = Dev(case.cones, case.s, case.z, ipm.PRIMAL_DUAL, case.mu)
    got = dev.step_length_ns(case.dz, case.ds, case.z, case.s, **case.scal)
    want = ns.step_length_sequential(case.cones, case.z, case.s, case.dz, case.ds, **case.scal)
    if excluded:
        visited, a = {0.0}, 0.5 if kind == "symmetric" else 1.0 - ns.SQRT_EPS
        while a >= ns.ALPHA_MIN:
            visited.add(a)
            a *= ns.BACKTRACK_STEP
        assert got in visited
        return
    assert got == want, (name, kind, seed, got, want)
    if kind == "free":
        assert got == 1.0 - ns.SQRT_EPS
    elif kind == "symmetric":
        assert got == 0.5
    elif kind == "zero":
        assert got == 0.0
    else:
        assert 0.0 < got <= (1.0 - ns.SQRT_EPS) * ns.BACKTRACK_STEP ** 2


def test_step_length_other_search_parameters_and_a_nan_point():
    """another backtrack_step / alpha_min pair against the host; a NaN step is not in the cone: 0, and the call ends"""
    case, _ = _step_case("mixed", "dual", 1)
    dev = Dev(case.cones, case.s, case.z, ipm.PRIMAL_DUAL, case.mu)
    for step, amin in ((0.5, 1e-3), (0.9, 0.3)):
        want = ns.step_length_sequential(case.cones, case.z, case.s, case.dz, case.ds, step=step, amin=amin)
        assert dev.step_length_ns(case.dz, case.ds, case.z, case.s, step=step, amin=amin) == want
    dz = case.dz.copy()
    dz[case.ns()[0][1]] = np.nan
    assert dev.step_length_ns(dz, case.ds, case.z, case.s) == 0.0
    assert dev.step_length_ns(dz, case.ds, case.z, case.s, step=0.999, amin=1e-12) == 0.0      # ~27600 trips, then the end


@pytest.mark.parametrize("name", ns.LISTS)
def test_barrier(name):
    case = ns.Case(name, seed=1)
    dev = Dev(case.cones, case.s, case.z, ipm.DUAL, case.mu)
    for alpha in ns.BARRIER_ALPHAS:
        bar, dot = dev.barrier(case.z, case.s, case.dz, case.ds, alpha)
        total, bound = ns.barrier_sum(ns.barrier_terms(case.cones, case.z, case.s, case.dz, case.ds, alpha), ns.DEVICE_FACTOR)
        assert math.isfinite(total)
        _note("barrier", abs(bar - total) / bound)
        assert abs(bar - total) <= bound, (name, alpha, bar, total, bound)
        zp, sp_ = case.z + alpha * case.dz, case.s + alpha * case.ds
        hi, lo = ir.dot_exact(zp, sp_)
        _note("dot", abs((dot - hi) - lo) / ir.dot_bound(zp, sp_))
        assert abs((dot - hi) - lo) <= ir.dot_bound(zp, sp_), (name, alpha, dot, hi)
    # a step that leaves a cone: a non-finite barrier is a result (the call returned HIPKKT_OK)
    for c, o in case.ns()[:1] + [(c, o) for c, o in zip(case.cones, case.off) if not ns.is_ns(c) and not isinstance(c, ZeroConeT)]:
        dz = case.dz.copy()
        dz[o:o + c.numel] = -2.0 * case.z[o:o + c.numel]
        if isinstance(c, SecondOrderConeT):                            # (-z has a positive residual too: shrink z0 below ||z1||)
            dz[o:o + c.numel] = 0.0
            dz[o] = 0.1 * np.linalg.norm(case.z[o + 1:o + c.numel]) - case.z[o]
        bar, dot = dev.barrier(case.z, case.s, dz, case.ds, 1.0)
        assert not math.isfinite(bar), (name, type(c).__name__, bar)
        assert math.isfinite(dot)


def test_refusals():
    """HIPKKT_ERR_ARG and nothing written: a generalized power cone in the handle, a deferred-status handle, a call before
    system.update (all but the unit initialisation), and step_length_ns with a backtrack_step of 0, 1 or 1.5 or an
    alpha_min of 0"""
    import torch
    from cuclarabel_amd import _lib

    def buffers(m):
        o = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
        o2 = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
        a = torch.ones(m, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return o, o2, a

    def refused(dev, needs_scaling_only=False, step_args=(0.8, 1e-4), only_step=False):
        L, h = _lib.lib(), dev.ks._h
        o, o2, a = buffers(dev.m)
        P = lambda t: t.data_ptr()
        alpha, bar = np.full(1, 7.0), np.full(2, 7.0)
        calls = [lambda: L.hipkkt_kkt_system_step_length_ns(h, P(a), P(a), P(a), P(a), 1.0, 1.0, 1.0, 1.0, step_args[0],
                                                            step_args[1], _lib.ptr(alpha))]
        if not only_step:
            calls += [lambda: L.hipkkt_kkt_system_affine_ds_ns(h, P(o), P(a)),
                      lambda: L.hipkkt_kkt_system_combined_ds_ns(h, P(o), P(a), P(a), P(a), P(a), 0.1, 1.0),
                      lambda: L.hipkkt_kkt_system_barrier(h, P(a), P(a), P(a), P(a), 0.5, _lib.ptr(bar))]
            if not needs_scaling_only:
                calls.append(lambda: L.hipkkt_kkt_system_unit_initialization(h, P(o), P(o2)))
        for call in calls:
            assert call() == -1, L.hipkkt_last_error()                 # HIPKKT_ERR_ARG
            assert L.hipkkt_last_error()
        dev.ks.synchronize()
        assert np.all(o.cpu().numpy() == 7.0) and np.all(o2.cpu().numpy() == 7.0) and alpha[0] == 7.0 and np.all(bar == 7.0), \
            "a refused call wrote something"

    refused(Dev([NonnegativeConeT(3), GenPowerConeT((0.5, 0.5), 1), ExponentialConeT()]))
    refused(Dev(ns._list("mixed")), needs_scaling_only=True)           # before update
    case = ns.Case("mixed", seed=1)
    dev = Dev(case.cones, case.s, case.z)
    dev.ks.set_deferred_status(True)
    refused(dev)
    dev.ks.set_deferred_status(False)
    assert dev.ks.deferred_status() in (0, 1, 2)
    for step_args in ((0.0, 1e-4), (1.0, 1e-4), (1.5, 1e-4), (0.8, 0.0), (float("nan"), 1e-4), (0.8, float("nan"))):
        refused(dev, step_args=step_args, only_step=True)
    assert dev.step_length_ns(0.01 * case.z, 0.01 * case.s, case.z, case.s) == 1.0 - ns.SQRT_EPS     # and works afterwards
    # the existing symmetric entry points still refuse this handle
    o, _, a = buffers(dev.m)
    assert _lib.lib().hipkkt_kkt_system_affine_ds(dev.ks._h, o.data_ptr()) == -1
