"""The 14 level-C cone-operation entry points (the symmetric four, the _ns five, the _gp five) against the three families
of handles, at the smallest cone lists that tell the families apart:

    a   nonnegative(1) + second-order(3)
    b   a + one exponential cone
    c   a + one generalized power cone, alpha = (0.5, 0.5), dim2 = 1

What each entry point accepts is the literal table ACCEPTS below: the symmetric four refuse a handle with an exponential,
power or generalized power cone, the _ns five one with a generalized power cone, the _gp five none.  A refused call
returns HIPKKT_ERR_ARG with a text that begins with the entry point's own name.  Where two families accept a handle
their results are the same bits: here every per-family kernel runs over zero cones or one, which is where a wrong offset
into the shared partial array would show.  Last, step_length_gp and barrier_gp on four small generalized power cones
(one full workgroup of the wave-per-cone kernels) and on five (one wave spills into a second workgroup), with no
lane-per-cone workgroup in front of their slots, against tests/genpow_step_reference.py under that module's bounds."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from cuclarabel_amd import ipm, _lib
from cuclarabel_amd.cones import NonnegativeConeT, SecondOrderConeT, ExponentialConeT, GenPowerConeT
from tests import iterate_reference as ir
from tests import nonsymmetric_reference as nr
from tests import nonsym_step_reference as ns
from tests import genpow_reference as gr
from tests import genpow_step_reference as gs
from tests.test_gpu_genpow_step_ops import Dev

pytestmark = pytest.mark.gpu

_BASE = [NonnegativeConeT(1), SecondOrderConeT(3)]
HANDLES = {"a": _BASE, "b": _BASE + [ExponentialConeT()], "c": _BASE + [GenPowerConeT((0.5, 0.5), 1)]}

FAMILY = {"hipkkt_kkt_system_affine_ds": "sym", "hipkkt_kkt_system_combined_ds": "sym", "hipkkt_kkt_system_step_length": "sym",
          "hipkkt_kkt_system_shift_to_interior": "sym",
          "hipkkt_kkt_system_unit_initialization": "ns", "hipkkt_kkt_system_affine_ds_ns": "ns",
          "hipkkt_kkt_system_combined_ds_ns": "ns", "hipkkt_kkt_system_step_length_ns": "ns", "hipkkt_kkt_system_barrier": "ns",
          "hipkkt_kkt_system_unit_initialization_gp": "gp", "hipkkt_kkt_system_affine_ds_gp": "gp",
          "hipkkt_kkt_system_combined_ds_gp": "gp", "hipkkt_kkt_system_step_length_gp": "gp", "hipkkt_kkt_system_barrier_gp": "gp"}
ACCEPTS = {"a": ("sym", "ns", "gp"), "b": ("ns", "gp"), "c": ("gp",)}


def _point(cones, seed):
    """an interior (s, z) and a step (dz, ds), cone by cone as the reference modules' Case classes fill theirs"""
    rng = np.random.default_rng([seed, 31])
    off = ns.offsets(cones)
    m = sum(c.numel for c in cones)
    s, z = np.zeros(m), np.zeros(m)
    for c, o in zip(cones, off):
        r = slice(o, o + c.numel)
        if isinstance(c, NonnegativeConeT):
            s[r], z[r] = np.exp(rng.normal(size=c.numel)), np.exp(rng.normal(size=c.numel))
        elif isinstance(c, SecondOrderConeT):
            for v in (s, z):
                t = rng.normal(size=c.numel)
                t[0] = np.linalg.norm(t[1:]) + np.exp(rng.normal())
                v[r] = t
        else:
            s[r], z[r] = (gr if gs.is_gp(c) else nr).random_interior_pair(c, rng)
    mu = float(s @ z) / sum(ipm._make_cones([c])[0].degree for c in cones)
    return SimpleNamespace(cones=cones, off=off, m=m, s=s, z=z, mu=mu, dz=0.1 * rng.normal(size=m), ds=0.1 * rng.normal(size=m))


_DEVS = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _DEVS.clear()


def _dev(key):
    """one handle per list, scaled once at its point"""
    if key not in _DEVS:
        pt = _point(HANDLES[key], 3)
        _DEVS[key] = (pt, Dev(pt.cones, pt.s, pt.z, ipm.DUAL, pt.mu))
    return _DEVS[key]


@pytest.mark.parametrize("key", sorted(HANDLES))
def test_every_entry_point_accepts_or_refuses_by_its_family(key):
    pt, dev = _dev(key)
    L, h = _lib.lib(), dev.ks._h
    # the tensors live to the end of the test: four inputs, two outputs, and a vector to shift in place
    keep = [dev.up(v) for v in (pt.s, pt.z, pt.dz, pt.ds)] + [dev.out(), dev.out(), dev.up(pt.s)]
    s, z, dz, ds, o, o2, v = (t.data_ptr() for t in keep)
    a1, a2 = np.zeros(1), np.zeros(2)
    calls = {
        "hipkkt_kkt_system_affine_ds": lambda f: f(h, o),
        "hipkkt_kkt_system_combined_ds": lambda f: f(h, o, dz, ds, 0.3, 0.7),
        "hipkkt_kkt_system_step_length": lambda f: f(h, dz, ds, z, s, 1.0, 1.0, 1.0, 1.0, _lib.ptr(a1)),
        "hipkkt_kkt_system_shift_to_interior": lambda f: f(h, v, 1, _lib.ptr(a2)),
    }
    for sfx in ("_ns", "_gp"):
        tail = "" if sfx == "_ns" else sfx                               # (unit_initialization and barrier carry no _ns)
        calls["hipkkt_kkt_system_unit_initialization" + tail] = lambda f: f(h, o, o2)
        calls["hipkkt_kkt_system_affine_ds" + sfx] = lambda f: f(h, o, s)
        calls["hipkkt_kkt_system_combined_ds" + sfx] = lambda f: f(h, o, dz, ds, s, z, 0.3, 0.7)
        calls["hipkkt_kkt_system_step_length" + sfx] = lambda f: f(h, dz, ds, z, s, 1.0, 1.0, 1.0, 1.0, gs.BACKTRACK_STEP,
                                                                   gs.ALPHA_MIN, _lib.ptr(a1))
        calls["hipkkt_kkt_system_barrier" + tail] = lambda f: f(h, z, s, dz, ds, 0.01, _lib.ptr(a2))
    assert sorted(calls) == sorted(FAMILY)
    for name, call in calls.items():
        rc = call(getattr(L, name))
        if FAMILY[name] in ACCEPTS[key]:
            assert rc == 0, (key, name, L.hipkkt_last_error())
        else:
            assert rc == -1, (key, name, rc)                             # HIPKKT_ERR_ARG
            assert L.hipkkt_last_error().decode().startswith(name + ":"), (key, name, L.hipkkt_last_error())
    dev.ks.synchronize()


def test_symmetric_list_ns_and_gp_rows_are_the_symmetric_entry_points_bits():
    pt, dev = _dev("a")
    want = dev.sym_ds(None, None, 0.0, 0.0, False)
    assert dev.affine_ds_ns(pt.s).tobytes() == want.tobytes()
    assert dev.affine_ds_gp(pt.s).tobytes() == want.tobytes()
    for sigma_mu, m_corr in ((0.3, 0.7), (0.0, 1.0)):
        want = dev.sym_ds(pt.dz, pt.ds, sigma_mu, m_corr, True)
        assert dev.combined_ds_ns(pt.dz, pt.ds, pt.s, pt.z, sigma_mu, m_corr).tobytes() == want.tobytes()
        assert dev.combined_ds_gp(pt.dz, pt.ds, pt.s, pt.z, sigma_mu, m_corr).tobytes() == want.tobytes()


def test_one_exponential_cone_gp_calls_are_their_ns_twins_bits():
    pt, dev = _dev("b")
    for x, y in zip(dev.unit_initialization_gp(), dev.unit_initialization()):
        assert x.tobytes() == y.tobytes()
    assert dev.affine_ds_gp(pt.s).tobytes() == dev.affine_ds_ns(pt.s).tobytes()
    assert dev.combined_ds_gp(pt.dz, pt.ds, pt.s, pt.z, 0.3, 0.7).tobytes() == \
        dev.combined_ds_ns(pt.dz, pt.ds, pt.s, pt.z, 0.3, 0.7).tobytes()
    # a free step and one that sends the exponential cone's search through its backtracks
    for dz in (0.01 * pt.z, pt.dz, -3.0 * pt.z):
        a = np.array([dev.step_length_gp(dz, pt.ds, pt.z, pt.s), dev.step_length_ns(dz, pt.ds, pt.z, pt.s)])
        assert a[:1].tobytes() == a[1:].tobytes(), a
    for alpha in gs.BARRIER_ALPHAS:
        assert np.array(dev.barrier_gp(pt.z, pt.s, pt.dz, pt.ds, alpha)).tobytes() == \
            np.array(dev.barrier(pt.z, pt.s, pt.dz, pt.ds, alpha)).tobytes()


def _gp_only(count):
    """`count` small generalized power cones alone; every cone steps along 0.01 (z, s) but the last, whose dual ray
    leaves its cone at a0 step^(1 + 1/2): the minimum is decided by the last cone's slot"""
    rng = np.random.default_rng([count, 32])
    pt = _point([gr.random_spec(rng, a, b) for a, b in gs.FIVE[:count]], count)
    pt.dz, pt.ds = 0.01 * pt.z, 0.01 * pt.s
    c, o = pt.cones[-1], pt.off[len(pt.cones) - 1]
    q = pt.z[o:o + c.numel]
    for _ in range(20):
        d = -q + 0.5 * np.abs(q).max() * rng.normal(size=c.numel) / math.sqrt(c.numel)
        t = ns._ray_exit(c, q, d, True)
        if t is not None and t > 1e-3:
            break
    else:
        raise AssertionError("no leaving direction found")
    pt.dz[o:o + c.numel] = d * (t / ((1.0 - gs.SQRT_EPS) * gs.BACKTRACK_STEP ** 1.5))
    return pt


@pytest.mark.parametrize("count", (4, 5))
def test_one_full_workgroup_of_generalized_power_cones_and_one_wave_more(count):
    pt = _gp_only(count)
    dev = Dev(pt.cones, pt.s, pt.z, ipm.DUAL, pt.mu)
    a0 = 1.0 - gs.SQRT_EPS
    assert not gs.step_length_ambiguous(pt.cones, pt.z, pt.s, pt.dz, pt.ds, a0), "the test's own point sits on a boundary"
    want = gs.step_length_sequential(pt.cones, pt.z, pt.s, pt.dz, pt.ds)
    assert want < a0 * gs.BACKTRACK_STEP, "the last cone does not bind"
    got = dev.step_length_gp(pt.dz, pt.ds, pt.z, pt.s)
    assert got == want, (count, got, want)
    dz, ds = 0.3 * pt.dz, 0.3 * pt.ds                                    # (short enough that BARRIER_ALPHAS stay interior)
    for alpha in gs.BARRIER_ALPHAS:
        bar, dot = dev.barrier_gp(pt.z, pt.s, dz, ds, alpha)
        total, bound = gs.barrier_reference(pt.cones, pt.z, pt.s, dz, ds, alpha, gs.DEVICE_FACTOR)
        assert math.isfinite(total)
        assert abs(bar - total) <= bound, (count, alpha, bar, total, bound)
        zp, sp_ = pt.z + alpha * dz, pt.s + alpha * ds
        hi, lo = ir.dot_exact(zp, sp_)
        assert abs((dot - hi) - lo) <= ir.dot_bound(zp, sp_), (count, alpha, dot, hi)
