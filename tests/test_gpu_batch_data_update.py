"""The member cost scalings on the device (hipkkt_kkt_system_set_equilibration_batch, hipkkt_kkt_system_update_data_P / _q
under it, hipkkt_kkt_system_data_norms_batch) against tests/batch_equilibration_reference.py, with == after every step:
K's values, the image the residual reads, q and b as tests/test_gpu_data_update.py reads them, -q through the initial
point.  The stacks are the model's (nb = 1; members of 1, 63, 64, 65, 255, 256, 257 x rows; a member without z rows; a
member without a stored entry of P; nb = 300 of two x rows), d, e and c_b each over eight decades."""
import numpy as np
import pytest

from tests import batch_equilibration_reference as be
from tests import data_update_reference as du
from tests import kvalue_reference as kv
from tests.test_gpu_data_update import Device, observe_without_negq

pytestmark = pytest.mark.gpu


class BatchDevice(Device):
    """tests/test_gpu_data_update.Device with the partition and the member costs under the model's method names"""

    def set_problems(self, blocks):
        self._refusable(self.system.set_problems, blocks)

    def set_equilibration_batch(self, d, e, c):
        from cuclarabel_amd import _lib
        c = _lib.f64(np.asarray(c, float).ravel())
        d = None if d is None else _lib.f64(d)
        e = None if e is None else _lib.f64(e)
        rc = _lib.lib().hipkkt_kkt_system_set_equilibration_batch(self.ks._h, _lib.ptr(d), _lib.ptr(e), _lib.ptr(c))
        if rc != 0:
            import re
            msg = _lib.lib().hipkkt_last_error().decode()
            assert rc == -1, (rc, msg)                           # HIPKKT_ERR_ARG, nothing else
            m = re.search(r"c\[(\d+)\]", msg)
            assert m is None or f"member {m.group(1)}" in msg    # the member is named
            raise du.Refused(msg, int(m.group(1)) if m else None)

    def data_norms_batch(self):
        return self._refusable(self.system.data_norms_batch)


def pair(name, seed=77, member_costs=True):
    case, blocks = be.stack_case(name)
    rng = np.random.default_rng(78)
    q, b = rng.standard_normal(case.n), rng.standard_normal(case.m)
    dev = BatchDevice(case, q, b)
    model = be.model_of_case(case, dev.ks.KKT(), dev.ks.maps())
    dev.observe_qb = lambda: observe_without_negq(dev, model)
    model.init(q, b)
    du.both(dev, model, "set_problems", blocks)
    d, e, c = du.scalings(case.n, case.m, seed)
    du.both(dev, model, "set_equilibration", d, e, c)
    if member_costs:
        du.both(dev, model, "set_equilibration_batch", d, e, be.member_costs(len(blocks), seed + 1))
    return case, blocks, dev, model


@pytest.mark.parametrize("name", list(be.STACKS))
def test_updates_of_P_and_q_under_member_costs(name):
    """vector and indexed (alternating between members, of length 1, of every entry) updates of P and q, _A and _b beside
    them; Kval, the image, q and b compared after every step"""
    case, blocks, dev, model = pair(name)
    if model.nb >= 2:
        assert model.cmem.max() / model.cmem.min() >= 1e7 and model.d.max() / model.d.min() >= 1e7
    be.sequence_member_updates(dev, model, case, 4000)
    got, want = dev.data_norms_batch(), model.data_norms_batch()
    assert be.same(got, want) and be.same(want, be.numpy_norms(model)), (got, want)


@pytest.mark.parametrize("name", list(be.STACKS))
def test_norms_are_numpys_maxima_member_by_member_and_a_nan_stays_in_its_member(name):
    case, blocks, dev, model = pair(name)
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 3))
    du.both(dev, model, "update_data", "b", du.new_values(case.m, 4))
    got = dev.data_norms_batch()
    assert got.shape == (model.nb, 2) and be.same(got, be.numpy_norms(model)), (got, be.numpy_norms(model))
    for b in range(model.nb):
        if model.z_off[b] == model.z_off[b + 1]:
            assert got[b, 1] == 0.0                              # a member without z rows
    # the maximum in a member's last row, then a NaN there
    victim = model.nb // 2
    last = np.array([model.x_off[victim + 1] - 1])
    du.both(dev, model, "update_data", "q", np.array([-1e300]), last)
    assert be.same(dev.data_norms_batch(), be.numpy_norms(model))
    du.both(dev, model, "update_data", "q", np.array([np.nan]), last)
    after = dev.data_norms_batch()
    assert np.isnan(after[victim, 0]) and be.same(after, be.numpy_norms(model))
    keep = np.ones(after.shape, bool)
    keep[victim, 0] = False
    assert np.array_equal(after[keep], got[keep]), "a NaN in one member's q shows there and nowhere else"
    # on a handle without member costs the handle's one c divides
    case, blocks, dev, model = pair(name, member_costs=False)
    assert be.same(dev.data_norms_batch(), be.numpy_norms(model))


def test_one_member_with_the_joint_c_is_the_scalar_call():
    """nb = 1, c_0 = c: every array equals that of the same data driven through the scalar set_equilibration"""
    case, blocks, dev, model = pair("one", member_costs=False)
    _, _, twin, tmodel = pair("one", member_costs=False)
    du.both(dev, model, "set_equilibration_batch", model.d, model.e, np.array([model.c]))
    for which in ("P", "q", "A", "b"):
        v = du.values_like(case.P.data, 8) if which == "P" else du.new_values(model.length(which), 9)
        for w in (dev, model, twin, tmodel):
            w.update_data(which, v)
        du.check(dev, model, which)
        du.check(twin, tmodel, which + " (scalar)")
        assert dev.ks.KKT().data.tobytes() == twin.ks.KKT().data.tobytes()
        for a, b in zip(Device.observe_qb(dev), Device.observe_qb(twin)):
            assert a is None or a.tobytes() == b.tobytes()
    assert tuple(dev.data_norms_batch()[0]) == twin.data_norms() == tmodel.data_norms()


def test_the_scalar_call_returns_the_handle_to_one_joint_c():
    case, blocks, dev, model = pair("no_z_no_P")
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 20))
    du.check(dev, model, "q under member costs")
    d, e, c = du.scalings(case.n, case.m, 5)
    du.both(dev, model, "set_equilibration", d, e, c)
    assert model.cmem is None
    v = du.values_like(case.P.data, 10)
    du.both(dev, model, "update_data", "P", v)
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 11))
    du.check(dev, model, "P, q after the scalar call")
    assert np.array_equal(model.Pval, v * (d[model.Prow] * d[model.Pcol]) * c)
    assert be.same(dev.data_norms_batch(), be.numpy_norms(model))
    du.both(dev, model, "set_problems", None)                    # ... and the partition may go again
    du.both(dev, model, "set_problems", blocks)
    du.both(dev, model, "set_equilibration_batch", None, None, be.member_costs(len(blocks), 3))      # d = e = NULL: ones
    assert (model.d == 1.0).all()
    du.both(dev, model, "update_data", "P", v)
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 12))
    du.check(dev, model, "P, q with scalings of one and member costs")


def test_negated_q_under_member_costs_reaches_the_constant_rhs_solves():
    """-q is read by the constant-RHS solve and the initial point only: after update_data_q under member costs the initial
    point equals, bit for bit, that of a second handle which got the model's scaled vectors through init"""
    case, blocks = be.stack_case("one")
    rng = np.random.default_rng(78)
    q, b = rng.standard_normal(case.n), rng.standard_normal(case.m)
    dev = BatchDevice(case, q, b)
    model = be.model_of_case(case, dev.ks.KKT(), dev.ks.maps())
    dev.observe_qb = lambda: observe_without_negq(dev, model)
    model.init(q, b)
    du.both(dev, model, "set_problems", blocks)
    d, e, _ = du.scalings(case.n, case.m, 7, lo=0.5, hi=2.0)
    du.both(dev, model, "set_equilibration_batch", d, e, np.array([3.7]))
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 31))
    du.both(dev, model, "update_data", "q", du.new_values(2, 32), np.array([case.n - 1, 0]))
    du.check(dev, model, "q")
    twin = Device(case, model.q, model.b)
    pts = []
    for w in (dev, twin):
        w.system_update(*case.hs(0))
        w.system.staging = "torch"
        ok, x, s, z = w.system.solve_initial_point()
        assert ok
        pts.append((x, s, z))
    for a, b_ in zip(*pts):
        assert a.tobytes() == b_.tobytes()
    assert np.abs(pts[0][0]).max() > 0


def test_every_refusal_leaves_the_handle_as_it_was():
    case, blocks, dev, model = pair("edges")
    du.both(dev, model, "update_data", "P", du.values_like(case.P.data, 40))
    du.check(dev, model, "create")
    norms = dev.data_norms_batch()
    ones_n, ones_m = np.ones(case.n), np.ones(case.m)
    # c_b of 0, negative, inf (and NaN), the member named
    for bad, where in ((0.0, 0), (-1.0, 3), (np.inf, 6), (np.nan, 2)):
        c = np.ones(model.nb)
        c[where] = bad
        du.expect_refused(dev, model, f"c[{where}] = {bad}", lambda w, c=c: w.set_equilibration_batch(ones_n, ones_m, c), pos=where)
    # one pointer missing, c missing
    du.expect_refused(dev, model, "e missing", lambda w: w.set_equilibration_batch(ones_n, None, np.ones(model.nb)))
    from cuclarabel_amd import _lib
    assert _lib.lib().hipkkt_kkt_system_set_equilibration_batch(dev.ks._h, _lib.ptr(ones_n), _lib.ptr(ones_m), None) == -1
    # set_problems while member costs are held: replace and clear
    du.expect_refused(dev, model, "set_problems (replace)", lambda w: w.set_problems(blocks))
    du.expect_refused(dev, model, "set_problems (clear)", lambda w: w.set_problems(None))
    # ... the scalings and the member costs are still the old ones
    du.both(dev, model, "update_data", "P", du.values_like(case.P.data, 41))
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 42))
    du.check(dev, model, "after the refusals")
    assert be.same(dev.data_norms_batch(), model.data_norms_batch()) and not be.same(dev.data_norms_batch(), norms)
    # a deferred-status handle
    dev.ks.set_deferred_status(True)
    model.deferred = True
    try:
        for w in (dev, model):
            with pytest.raises(du.Refused):
                w.set_equilibration_batch(ones_n, ones_m, np.ones(model.nb))
            with pytest.raises(du.Refused):
                w.data_norms_batch()
    finally:
        dev.ks.set_deferred_status(False)
        model.deferred = False
    du.both(dev, model, "update_data", "P", du.values_like(case.P.data, 44))
    du.check(dev, model, "after the deferred refusals")
    assert be.same(dev.data_norms_batch(), model.data_norms_batch())


def test_no_partition_is_refused():
    case, blocks = be.stack_case("no_z_no_P")
    rng = np.random.default_rng(78)
    q, b = rng.standard_normal(case.n), rng.standard_normal(case.m)
    dev = BatchDevice(case, q, b)
    model = be.model_of_case(case, dev.ks.KKT(), dev.ks.maps())
    dev.observe_qb = lambda: observe_without_negq(dev, model)
    model.init(q, b)
    d, e, c = du.scalings(case.n, case.m, 9)
    du.both(dev, model, "set_equilibration", d, e, c)
    du.expect_refused(dev, model, "no partition", lambda w: w.set_equilibration_batch(d, e, np.ones(len(blocks))))
    for w in (dev, model):
        with pytest.raises(du.Refused):
            w.data_norms_batch()
    du.both(dev, model, "update_data", "P", du.values_like(case.P.data, 50))      # the joint c is still in force
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 51))
    du.check(dev, model, "after the refusals")
    assert dev.data_norms() == model.data_norms()
