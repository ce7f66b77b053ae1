"""The host model of the member cost scalings (tests/batch_equilibration_reference.py) and the design of the sequence that
tests/test_gpu_batch_data_update.py runs on the device -- no GPU.  The pattern and the maps are the oracle's.

  - a fault-free model passes the sequence on every stack, and its products are numpy float64 in the stated order (==);
  - every seeded fault is caught;
  - with nb = 1 and c_0 = c the model equals the scalar model; after the scalar set_equilibration the joint c is back;
  - the norms equal numpy's maxima member by member, a NaN shows in its member alone;
  - the refusals change nothing."""
import numpy as np
import pytest

from tests import batch_equilibration_reference as be
from tests import data_update_reference as du
from tests import kvalue_reference as kv
from tests.oracle_bindings import OracleKKT

_CASES = {}


def case_and_oracle(name):
    if name not in _CASES:
        case, blocks = be.stack_case(name)
        _CASES[name] = (case, blocks, OracleKKT(case.P, case.A, case.cones))
    return _CASES[name]


def pair(name, bfault=None, member_costs=True, seed=77):
    """(case, device, model): a model with the fault standing in for the handle, and the fault-free one"""
    case, blocks, o = case_and_oracle(name)
    out = []
    for f in (bfault, None):
        mdl = be.model_of_case(case, o.K(), o.maps(), bfault=f)
        rng = np.random.default_rng(78)
        mdl.init(rng.standard_normal(case.n), rng.standard_normal(case.m))
        mdl.set_problems(blocks)
        d, e, c = du.scalings(case.n, case.m, seed)
        mdl.set_equilibration(d, e, c)
        if member_costs:
            mdl.set_equilibration_batch(d, e, be.member_costs(len(blocks), seed + 1))
        out.append(mdl)
    return case, out[0], out[1]


@pytest.mark.parametrize("name", list(be.STACKS))
def test_fault_free_model_passes_the_sequence_and_multiplies_in_the_stated_order(name):
    case, dev, model = pair(name)
    be.sequence_member_updates(dev, model, case, 4000)
    # the products, restated with numpy float64 in the stated order
    v, q = du.values_like(case.P.data, 1), du.new_values(case.n, 2)
    model.update_data("P", v)
    model.update_data("q", q)
    d, c = model.d, model.cmem
    r, col = model.Prow, model.Pcol
    assert np.array_equal(model.Pval, (v * (d[r] * d[col])) * c[model.xmem[r]])
    assert np.array_equal(model.q, (q * d) * c[model.xmem]) and np.array_equal(model.negq, -model.q)
    assert np.array_equal(model.xmem[r], model.xmem[col]), "a stored entry of P has its row and column in one member"
    if model.nb >= 2:
        assert c.max() / c.min() >= 1e7 and model.d.max() / model.d.min() >= 1e7


def _inconsistent(m):
    """a row -> member table that splits coupled rows: the boundary of the first two members moved by one row"""
    m.xmem = m.xmem.copy()
    m.xmem[m.x_off[1]] = 0


@pytest.mark.parametrize("bfault", be.BFAULTS)
def test_every_seeded_fault_is_caught(bfault):
    case, dev, model = pair("edges", bfault)
    if bfault == "column_member":
        # with a consistent table the column's member IS the row's: the fault cannot show ...
        be.sequence_member_updates(dev, model, case, 4000)
        # ... so the table is made inconsistent, the same way for both
        _inconsistent(dev)
        _inconsistent(model)
        assert (model.xmem[model.Prow] != model.xmem[model.Pcol]).any()
        du.both(dev, model, "update_data", "P", du.values_like(case.P.data, 5))
        with pytest.raises(kv.ValuePathError) as err:
            du.check(dev, model, "P vector, inconsistent table")
        assert err.value.helper == "assert_values"
    elif bfault in ("joint_c", "c_before_d"):
        with pytest.raises(kv.ValuePathError):
            be.sequence_member_updates(dev, model, case, 4000)
        for which in ("P", "q"):                             # ... in P and in q alike
            case, dev, model = pair("edges", bfault)
            v = du.values_like(case.P.data, 6) if which == "P" else du.new_values(case.n, 7)
            du.both(dev, model, "update_data", which, v)
            with pytest.raises(kv.ValuePathError):
                du.check(dev, model, which)
    else:
        be.sequence_member_updates(dev, model, case, 4000)   # (the update path is fault-free)
        assert not be.same(dev.data_norms_batch(), model.data_norms_batch())
        assert be.same(model.data_norms_batch(), be.numpy_norms(model))
    if bfault == "joint_c":
        case, dev, model = pair("edges", bfault)
        assert not be.same(dev.data_norms_batch(), model.data_norms_batch())


def test_a_straddling_wave_is_where_the_fold_fault_shows():
    """members of 1 and 63 x rows share the first wave: the fold fault moves the second member's maximum into the first's
    word; on a stack whose boundaries all fall on multiples of 64 it cannot show"""
    case, dev, model = pair("edges", "straddle_fold")
    q = np.ones(case.n)
    q[5] = 1e6                                               # in member 1, rows 1..63, first wave
    for w in (dev, model):
        w.set_equilibration_batch(np.ones(case.n), np.ones(case.m), np.ones(w.nb))
        w.update_data("q", q)
    got, want = dev.data_norms_batch(), model.data_norms_batch()
    assert want[1, 0] == 1e6 and want[0, 0] == 1.0 and got[0, 0] == 1e6 and got[1, 0] != 1e6


@pytest.mark.parametrize("name", list(be.STACKS))
def test_norms_are_numpys_maxima_member_by_member_and_a_nan_stays_in_its_member(name):
    case, _, model = pair(name)
    model.update_data("q", du.new_values(case.n, 3))
    model.update_data("b", du.new_values(case.m, 4))
    got = model.data_norms_batch()
    assert got.shape == (model.nb, 2) and be.same(got, be.numpy_norms(model))
    for b in range(model.nb):
        if model.z_off[b] == model.z_off[b + 1]:
            assert got[b, 1] == 0.0                          # a member without z rows
    victim = model.nb // 2
    model.update_data("q", np.array([np.nan]), np.array([model.x_off[victim + 1] - 1]))
    after = model.data_norms_batch()
    assert np.isnan(after[victim, 0]) and be.same(after, be.numpy_norms(model))
    keep = np.ones(after.shape, bool)
    keep[victim, 0] = False
    assert np.array_equal(after[keep], got[keep])
    # without member costs the handle's one c divides every member's norm
    case, _, model = pair(name, member_costs=False)
    assert be.same(model.data_norms_batch(), be.numpy_norms(model))
    assert model.data_norms_batch()[0, 0] == np.abs(model.q * (1.0 / model.d))[:model.x_off[1]].max() / model.c


def test_one_member_with_the_joint_c_is_the_scalar_model():
    case, _, model = pair("one", member_costs=False)
    _, _, twin = pair("one", member_costs=False)
    model.set_equilibration_batch(model.d, model.e, np.array([model.c]))
    for which in ("P", "q", "A", "b"):
        v = du.values_like(case.P.data, 8) if which == "P" else du.new_values(model.length(which), 9)
        du.both(model, twin, "update_data", which, v)
        du.check(model, twin, which)
    assert tuple(model.data_norms_batch()[0]) == twin.data_norms()


def test_the_scalar_call_returns_the_handle_to_one_joint_c():
    case, dev, model = pair("edges")
    d, e, c = du.scalings(case.n, case.m, 5)
    model.set_equilibration(d, e, c)
    assert model.cmem is None
    v = du.values_like(case.P.data, 10)
    model.update_data("P", v)
    model.update_data("q", du.new_values(case.n, 11))
    assert np.array_equal(model.Pval, v * (d[model.Prow] * d[model.Pcol]) * c)
    assert np.array_equal(model.q, du.new_values(case.n, 11) * d * c)
    model.set_problems(None)                                 # ... and the partition may go again


def test_refusals_leave_the_model_unchanged_and_name_the_member():
    case, blocks, o = case_and_oracle("edges")
    fresh = be.model_of_case(case, o.K(), o.maps())
    fresh.init(np.zeros(case.n), np.zeros(case.m))
    with pytest.raises(du.Refused):
        fresh.set_equilibration_batch(np.ones(case.n), np.ones(case.m), np.ones(len(blocks)))       # no partition
    with pytest.raises(du.Refused):
        fresh.data_norms_batch()
    case, dev, model = pair("edges")
    before = (model.d.copy(), model.e.copy(), model.cmem.copy(), model.c)
    for bad, where in ((0.0, 0), (-1.0, 3), (np.inf, 6), (np.nan, 2)):
        c = np.ones(model.nb)
        c[where] = bad
        c[-1] = bad if where == 6 else 1.0
        with pytest.raises(du.Refused) as err:
            model.set_equilibration_batch(np.ones(case.n), np.ones(case.m), c)
        assert err.value.pos == where
    with pytest.raises(du.Refused):
        model.set_problems(blocks)                           # member costs are held: replace ...
    with pytest.raises(du.Refused):
        model.set_problems(None)                             # ... or clear
    model.deferred = True
    with pytest.raises(du.Refused):
        model.set_equilibration_batch(np.ones(case.n), np.ones(case.m), np.ones(model.nb))
    with pytest.raises(du.Refused):
        model.data_norms_batch()
    model.deferred = False
    after = (model.d, model.e, model.cmem, model.c)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and model.nb == len(blocks)
    du.check(dev, model, "after the refusals")
