"""The device cone operations between the solves on cone lists that hold generalized power cones
(hipkkt_kkt_system_unit_initialization_gp / _affine_ds_gp / _combined_ds_gp / _step_length_gp / _barrier_gp:
csrc/step_kernels.hip) against tests/genpow_step_reference.py.

Cone lists (genpow_step_reference.LISTS): single cones at the wave edges (1,1) .. (65,2), on both sides of the
one-wave limit of 512 rows, workgroup walks of 3 and 5 strides, five small cones (a partly filled workgroup of four
waves), and generalized power cones among all six other kinds.  Every call is made twice and must repeat bit for bit;
inputs must come back unchanged; the rows of the other cones must equal, bit for bit, what the _ns entry points give on
a twin handle without the generalized power cones.  Worst error / bound ratios are printed under -s."""
import math

import numpy as np
import pytest

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import NonnegativeConeT, PSDTriangleConeT, GenPowerConeT
from tests import iterate_reference as ir
from tests import genpow_step_reference as gs
from tests import test_gpu_nonsym_step_ops as base

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _DEVS.clear()                                                         # (the shared handles go with the module, not with the interpreter)
    print("\nworst device error / bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), float(r))


class Dev(base.Dev):
    """base.Dev (a level-C handle over a cone list, scaled at (s, z) unless s is None) with the _gp calls"""

    def unit_initialization_gp(self):
        def run():
            s, z = self.out(), self.out()
            assert self.system.unit_initialization_gp_dev(s.data_ptr(), z.data_ptr())
            return np.r_[self.down(s)[:self.m], self.down(z)[:self.m]]
        r = self.twice(run)
        return r[:self.m], r[self.m:]

    def affine_ds_gp(self, s):
        ts = self.up(s)

        def run():
            o = self.out()
            assert self.system.affine_ds_gp_dev(o.data_ptr(), ts.data_ptr())
            return self.down(o)[:self.m]
        got = self.twice(run)
        self.unchanged([(ts, s)])
        return got

    def combined_ds_gp(self, dz, ds, s, z, sigma_mu, m_corr):
        t = [self.up(v) for v in (dz, ds, s, z)]

        def run():
            o = self.out()
            assert self.system.combined_ds_gp_dev(o.data_ptr(), *[v.data_ptr() for v in t], sigma_mu, m_corr)
            return self.down(o)[:self.m]
        got = self.twice(run)
        self.unchanged(zip(t, (dz, ds, s, z)))
        return got

    def step_length_gp(self, dz, ds, z, s, step=gs.BACKTRACK_STEP, amin=gs.ALPHA_MIN, **scal):
        t = [self.up(v) for v in (dz, ds, z, s)]
        got = float(self.twice(lambda: self.system.step_length_gp_dev(
            *[v.data_ptr() for v in t], scal.get("dtau", 1.0), scal.get("dkappa", 1.0), scal.get("tau", 1.0),
            scal.get("kappa", 1.0), step, amin)))
        self.unchanged(zip(t, (dz, ds, z, s)))
        return got

    def barrier_gp(self, z, s, dz, ds, alpha):
        t = [self.up(v) for v in (z, s, dz, ds)]
        got = self.twice(lambda: np.array(self.system.barrier_gp_dev(*[v.data_ptr() for v in t], alpha)))
        self.unchanged(zip(t, (z, s, dz, ds)))
        return float(got[0]), float(got[1])


_DEVS = {}


def _dev(name):
    """one scaled handle (and its twin without the generalized power cones) per list, shared by the tests"""
    if name not in _DEVS:
        case = gs.Case(name)
        dev = Dev(case.cones, case.s, case.z, ipm.DUAL, case.mu)
        others, rows = case.twin()
        twin = Dev(others, case.s[rows], case.z[rows], ipm.DUAL, case.mu) if others else None
        _DEVS[name] = (case, dev, twin, rows)
    return _DEVS[name]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gs.LISTS)
def test_unit_initialization(name):
    """sqrt is correctly rounded: numpy's bits on the generalized power rows; the other rows as the _ns call; no scaling"""
    case = gs.Case(name)
    s, z = Dev(case.cones).unit_initialization_gp()
    assert s.tobytes() == z.tobytes()
    for c, o in case.gp():
        assert s[o:o + c.numel].tobytes() == gs.unit_start(c).tobytes(), (name, o)
    others, rows = case.twin()
    if others:
        ts, tz = Dev(others).unit_initialization()
        assert s[rows].tobytes() == ts.tobytes() and z[rows].tobytes() == tz.tobytes()


@pytest.mark.parametrize("name", gs.LISTS)
def test_affine_and_combined_ds(name):
    case, dev, twin, rows = _dev(name)
    gp = ~rows
    got = dev.affine_ds_gp(case.s)
    assert got[gp].tobytes() == case.s[gp].tobytes(), "affine_ds_gp: the generalized power rows are a copy of s"
    if twin:
        assert got[rows].tobytes() == twin.affine_ds_ns(case.s[rows]).tobytes(), "affine_ds_gp: the other rows"
    grads = dev.ks.genpow()                                               # the device's own stored gradient
    for sigma_mu, m_corr in ((0.3, 0.7), (0.0, 1.0)):
        got = dev.combined_ds_gp(case.dz, case.ds, case.s, case.z, sigma_mu, m_corr)
        if twin:
            want = twin.combined_ds_ns(case.dz[rows], case.ds[rows], case.s[rows], case.z[rows], sigma_mu, m_corr)
            assert got[rows].tobytes() == want.tobytes(), "combined_ds_gp: the other rows differ from hipkkt_kkt_system_combined_ds_ns"
        for (c, o), (g, *_) in zip(case.gp(), grads):
            r = slice(o, o + c.numel)
            # one rounding of the product and one of the sum, or a single one where they are fused: 2 u (|s_i| + |sigma_mu g_i|) covers both
            err = np.abs(got[r] - (case.s[r] + sigma_mu * g))
            bound = 2.0 * gs.U * (np.abs(case.s[r]) + np.abs(sigma_mu * g))
            _note("combined_ds", (err / np.where(bound > 0, bound, 1.0)).max())
            assert np.all(err <= bound), (name, o, sigma_mu)
        # step_z, step_s and m_corr are not read on the generalized power rows
        other = dev.combined_ds_gp(case.dz * 3.0 + 1.0, case.ds - 2.0, case.s, case.z, sigma_mu, 0.25)
        assert other[gp].tobytes() == got[gp].tobytes()


_STEP_PARAMS = [(name, kind) for name in gs.LISTS for kind in gs.STEP_KINDS]


@pytest.mark.parametrize("name,kind", _STEP_PARAMS)
def test_step_length(name, kind):
    """equal as doubles to the host's sequential composite rule"""
    case, excluded = gs.step_cases()[(name, kind)]
    _, dev, _, _ = _dev(name)                                             # (the same cones and the same (s, z): the scaling is the case's)
    assert [c.numel for c in dev.cones] == [c.numel for c in case.cones]
    got = dev.step_length_gp(case.dz, case.ds, case.z, case.s, **case.scal)
    if excluded:
        visited, a = {0.0}, 1.0 - gs.SQRT_EPS
        while a >= gs.ALPHA_MIN:
            visited.add(a)
            a *= gs.BACKTRACK_STEP
        assert got in visited
        return
    want = gs.step_length_sequential(case.cones, case.z, case.s, case.dz, case.ds, **case.scal)
    assert got == want, (name, kind, got, want)


def test_step_length_symmetric_start_other_parameters_nan_and_cone_order():
    case, _ = gs.step_cases()[("mixed", "dual1")]
    _, dev, _, _ = _dev("mixed")
    # a nonnegative row sets the common start to exactly 0.5: the searches begin there
    dz = case.dz.copy()
    nn = [o for c, o in zip(case.cones, case.off) if isinstance(c, NonnegativeConeT)][0]
    dz[nn] = -case.z[nn] / 0.5
    assert dev.step_length_gp(dz, case.ds, case.z, case.s) == gs.step_length_sequential(case.cones, case.z, case.s, dz, case.ds)
    assert dev.step_length_gp(dz, case.ds, case.z, case.s, dtau=-4.0) == \
        gs.step_length_sequential(case.cones, case.z, case.s, dz, case.ds, dtau=-4.0)
    for step, amin in ((0.5, 1e-3), (0.9, 0.3)):
        want = gs.step_length_sequential(case.cones, case.z, case.s, case.dz, case.ds, step=step, amin=amin)
        assert dev.step_length_gp(case.dz, case.ds, case.z, case.s, step=step, amin=amin) == want
    # a NaN in a generalized power row: not in the cone, 0 -- on a small cone and on one that takes a workgroup
    for nm in ("mixed", "300x800"):
        cs, d, _, _ = _dev(nm)
        c, o = cs.gp()[-1]
        for row in (o, o + c.numel - 1):
            for which in (0, 1):
                vz, vs = 0.01 * cs.z, 0.01 * cs.s
                (vz, vs)[which][row] = np.nan
                assert d.step_length_gp(vz, vs, cs.z, cs.s) == 0.0
    dz = case.dz.copy()
    dz[case.gp_rows()] = np.nan
    assert dev.step_length_gp(dz, case.ds, case.z, case.s, step=0.999, amin=1e-12) == 0.0      # ~27600 trips, then the end
    # the cone order alone changes nothing
    want = dev.step_length_gp(case.dz, case.ds, case.z, case.s)
    order = np.random.default_rng(5).permutation(len(case.cones))
    pc = case.permuted(order)
    pdev = Dev(pc.cones, pc.s, pc.z, ipm.DUAL, pc.mu)
    assert pdev.step_length_gp(pc.dz, pc.ds, pc.z, pc.s) == want


@pytest.mark.parametrize("name", gs.LISTS)
def test_barrier(name):
    case, dev, _, _ = _dev(name)
    for alpha in gs.BARRIER_ALPHAS:
        bar, dot = dev.barrier_gp(case.z, case.s, case.dz, case.ds, alpha)
        total, bound = gs.barrier_reference(case.cones, case.z, case.s, case.dz, case.ds, alpha, gs.DEVICE_FACTOR)
        assert math.isfinite(total)
        _note("barrier", abs(bar - total) / bound)
        assert abs(bar - total) <= bound, (name, alpha, bar, total, bound)
        zp, sp_ = case.z + alpha * case.dz, case.s + alpha * case.ds
        hi, lo = ir.dot_exact(zp, sp_)
        _note("dot", abs((dot - hi) - lo) / ir.dot_bound(zp, sp_))
        assert abs((dot - hi) - lo) <= ir.dot_bound(zp, sp_), (name, alpha, dot, hi)
    # ||w|| just outside the dual cone: a non-finite barrier is a result (the call returned HIPKKT_OK)
    c, o = case.gp()[-1]
    phi, nw, _ = gs._phi_norm(c, case.z[o:o + c.numel], True)
    z = case.z.copy()
    z[o + c.dim1:o + c.numel] *= float((1.0001 * phi / nw) ** 0.5)
    bar, dot = dev.barrier_gp(z, case.s, 0.0 * case.dz, 0.0 * case.ds, 0.0)
    assert not math.isfinite(bar), (name, bar)
    assert math.isfinite(dot)
    # ||s[dim1:]|| = 0: the closed-form branch of the primal gradient
    s = case.s.copy()
    s[o + c.dim1:o + c.numel] = 0.0
    zero = np.zeros(case.m)
    bar, _ = dev.barrier_gp(case.z, s, zero, zero, 0.0)
    total, bound = gs.barrier_reference(case.cones, case.z, s, zero, zero, 0.0, gs.DEVICE_FACTOR)
    _note("barrier_closed_form", abs(bar - total) / bound)
    assert abs(bar - total) <= bound, (name, bar, total, bound)


def test_without_a_generalized_power_cone_the_calls_are_the_ns_calls():
    case = base.ns.Case("mixed", seed=1)
    dev = Dev(case.cones, case.s, case.z, ipm.DUAL, case.mu)
    s1, z1 = dev.unit_initialization_gp()
    s2, z2 = dev.unit_initialization()
    assert s1.tobytes() == s2.tobytes() and z1.tobytes() == z2.tobytes()
    assert dev.affine_ds_gp(case.s).tobytes() == dev.affine_ds_ns(case.s).tobytes()
    assert dev.combined_ds_gp(case.dz, case.ds, case.s, case.z, 0.3, 0.7).tobytes() == \
        dev.combined_ds_ns(case.dz, case.ds, case.s, case.z, 0.3, 0.7).tobytes()
    assert dev.step_length_gp(case.dz, case.ds, case.z, case.s) == dev.step_length_ns(case.dz, case.ds, case.z, case.s)
    assert dev.barrier_gp(case.z, case.s, case.dz, case.ds, 0.01) == dev.barrier(case.z, case.s, case.dz, case.ds, 0.01)


def test_refusals():
    """HIPKKT_ERR_ARG and nothing written: a deferred-status handle, a call before system.update (all but the unit
    start), a PSD cone of side 49, and step_length_gp with a backtrack_step of 0, 1 or 1.5 or an alpha_min of 0 or NaN"""
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
        calls = [lambda: L.hipkkt_kkt_system_step_length_gp(h, P(a), P(a), P(a), P(a), 1.0, 1.0, 1.0, 1.0, step_args[0],
                                                            step_args[1], _lib.ptr(alpha))]
        if not only_step:
            calls += [lambda: L.hipkkt_kkt_system_affine_ds_gp(h, P(o), P(a)),
                      lambda: L.hipkkt_kkt_system_combined_ds_gp(h, P(o), P(a), P(a), P(a), P(a), 0.1, 1.0),
                      lambda: L.hipkkt_kkt_system_barrier_gp(h, P(a), P(a), P(a), P(a), 0.5, _lib.ptr(bar))]
            if not needs_scaling_only:
                calls.append(lambda: L.hipkkt_kkt_system_unit_initialization_gp(h, P(o), P(o2)))
        for call in calls:
            assert call() == -1, L.hipkkt_last_error()                 # HIPKKT_ERR_ARG
            assert L.hipkkt_last_error()
        dev.ks.synchronize()
        assert np.all(o.cpu().numpy() == 7.0) and np.all(o2.cpu().numpy() == 7.0) and alpha[0] == 7.0 and np.all(bar == 7.0), \
            "a refused call wrote something"

    refused(Dev(gs.Case("mixed").cones), needs_scaling_only=True)      # before update
    refused(Dev([NonnegativeConeT(2), GenPowerConeT((0.5, 0.5), 1), PSDTriangleConeT(49)]))
    case, dev, _, _ = _dev("mixed")
    dev.ks.set_deferred_status(True)
    refused(dev)
    dev.ks.set_deferred_status(False)
    assert dev.ks.deferred_status() in (0, 1, 2)
    for step_args in ((0.0, 1e-4), (1.0, 1e-4), (1.5, 1e-4), (0.8, 0.0), (float("nan"), 1e-4), (0.8, float("nan"))):
        refused(dev, step_args=step_args, only_step=True)
    assert dev.step_length_gp(0.01 * case.z, 0.01 * case.s, case.z, case.s) == 1.0 - gs.SQRT_EPS     # and works afterwards
    # the _ns and the symmetric entry points still refuse this handle
    o, _, a = buffers(dev.m)
    assert _lib.lib().hipkkt_kkt_system_affine_ds_ns(dev.ks._h, o.data_ptr(), a.data_ptr()) == -1
    assert _lib.lib().hipkkt_kkt_system_affine_ds(dev.ks._h, o.data_ptr()) == -1
