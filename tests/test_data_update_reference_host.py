"""The host model of the data-updating path (tests/data_update_reference.py) and the design of the sequences that
tests/test_gpu_data_update.py runs on the device -- no GPU.  The pattern and the maps are the oracle's, which
test_assembly_maps_bit_exact pins as equal to the library's.

  - a fault-free model passes every sequence;
  - every seeded fault is caught by a sequence named here, by the helper named here;
  - the model's arithmetic is equilibrate.rescale_q / rescale_b's, and one round of the numpy Ruiz equilibration
    (tests/ref_equilibrate_numpy.py) leaves exactly what the model's updates with that round's (d, e, c) leave;
  - the model's index check names the places the library's is specified to name."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import data_update_reference as du
from tests import kvalue_reference as kv
from tests.oracle_bindings import OracleKKT

_CASES = {}


def case_and_oracle(name):
    if name not in _CASES:
        case = kv.SMALL_CASES[name]()
        _CASES[name] = (case, OracleKKT(case.P, case.A, case.cones))
    return _CASES[name]


def pair(name, fault=None, scaled=True):
    """(case, device, model): a model with the fault standing in for the handle, and the fault-free one"""
    case, o = case_and_oracle(name)
    out = []
    for f in (fault, None):
        mdl = du.model_of_case(case, o.K(), o.maps(), fault=f)
        if scaled:
            mdl.set_equilibration(*du.scalings(case.n, case.m, 77))
        rng = np.random.default_rng(78)
        mdl.init(rng.standard_normal(case.n), rng.standard_normal(case.m))
        out.append(mdl)
    return case, out[0], out[1]


@pytest.mark.parametrize("scaled", [True, False], ids=["scaled", "ones"])
@pytest.mark.parametrize("name", ["segments", "block_edge[246,10]"])
def test_fault_free_model_passes_every_sequence(name, scaled):
    case, dev, model = pair(name, scaled=scaled)
    du.run_all(dev, model, case)
    assert model.const_stale and not model.dirty


# fault -> (the sequence that must raise, the helper that raises)
EXPOSED_BY = {
    "scaling_operand": (du.sequence_vector_P, "assert_values"),
    "missing_negq": (du.sequence_qb, "check"),
    "through_while_dirty": (du.sequence_dirty_P, "assert_image"),
    "second_slot": (du.sequence_vector_P, "assert_image"),
    "stale_accepted": (du.sequence_indexed_A, "refusal"),
}


@pytest.mark.parametrize("fault", du.FAULTS)
def test_every_seeded_fault_is_caught(fault):
    assert set(EXPOSED_BY) == set(du.FAULTS)
    seq, helper = EXPOSED_BY[fault]
    case, dev, model = pair("segments", fault)
    with pytest.raises(kv.ValuePathError) as err:
        seq(dev, model, case, 4000)
    assert err.value.helper == helper, str(err.value)
    # ... and by the whole run, whatever comes first
    case, dev, model = pair("segments", fault)
    with pytest.raises(kv.ValuePathError):
        du.run_all(dev, model, case)


def test_scaling_operand_fault_shows_in_every_one_of_the_four():
    for which in ("P", "A", "q", "b"):
        case, dev, model = pair("segments", "scaling_operand")
        v = du.new_values(model.length(which), 5)
        du.both(dev, model, "update_data", which, v)
        with pytest.raises(kv.ValuePathError):
            du.check(dev, model, which)


def test_model_arithmetic_is_rescale_q_and_rescale_b():
    from cuclarabel_amd import equilibrate as eqm
    case, _, model = pair("segments")
    eq = eqm.Equilibration(model.d, 1.0 / model.d, model.e, 1.0 / model.e, model.c)
    q, b = du.new_values(case.n, 11), du.new_values(case.m, 12)
    model.update_data("q", q)
    model.update_data("b", b)
    assert np.array_equal(model.q, eqm.rescale_q(q, eq)) and np.array_equal(model.b, eqm.rescale_b(b, eq))
    assert np.array_equal(model.negq, -model.q)
    nq, nb = model.data_norms()
    assert nq == np.abs(model.q * eq.dinv).max() / eq.c and nb == np.abs(model.b * eq.einv).max()
    # the recovered norms are the unscaled vectors' to a few ulps (they are not exact: q d c dinv / c rounds four times)
    assert abs(nq - np.abs(q).max()) <= 8 * np.finfo(float).eps * np.abs(q).max()
    assert abs(nb - np.abs(b).max()) <= 8 * np.finfo(float).eps * np.abs(b).max()


def test_one_ruiz_round_leaves_what_the_model_leaves():
    """max_iter = 1 from d = e = 1: P <- fl(fl(P fl(d d)) c), A <- fl(A fl(e d)), q <- fl(fl(q d) c), b <- fl(b e) -- the
    update kernels' order.  Nonnegative and zero cones only, so that no per-cone correction follows."""
    from cuclarabel_amd.cones import NonnegativeConeT, ZeroConeT
    from tests.ref_equilibrate_numpy import equilibrate_ref
    rng = np.random.default_rng(21)
    n, m = 9, 14
    cones = [ZeroConeT(3), NonnegativeConeT(11)]
    case = kv.Case("ruiz", kv._tridiag_P(n, rng) * 37.0, kv._one_or_two_per_row(m, n, rng, 2) * 0.03, cones, 21)
    q, b = 5.0 * rng.standard_normal(n), rng.standard_normal(m)
    Ps, qs, As, bs, d, e, c = equilibrate_ref(case.P, q, case.A, b, cones, max_iter=1)
    assert c != 1.0 and not np.array_equal(d, np.ones(n))
    o = OracleKKT(case.P, case.A, cones)
    model = du.model_of_case(case, o.K(), o.maps())
    model.set_equilibration(d, e, c)
    model.init(np.zeros(n), np.zeros(m))
    for which, v in (("P", case.P.data), ("A", case.A.data), ("q", q), ("b", b)):
        model.update_data(which, v)
    assert np.array_equal(model.Pval, Ps.data) and np.array_equal(model.Aval, As.data)
    assert np.array_equal(model.q, qs) and np.array_equal(model.b, bs)
    assert np.array_equal(model.Kval[model.maps["P"]], Ps.data) and np.array_equal(model.Kval[model.maps["A"]], As.data)


def test_entry_coordinates_are_the_matrices_own():
    case, _, model = pair("segments")
    Pcol = np.repeat(np.arange(case.n), np.diff(case.P.indptr))
    Acol = np.repeat(np.arange(case.n), np.diff(case.A.indptr))
    assert np.array_equal(model.Prow, case.P.indices) and np.array_equal(model.Pcol, Pcol)
    assert np.array_equal(model.Arow, case.A.indices) and np.array_equal(model.Acol, Acol)
    assert (model.Prow != model.Pcol).any() and (model.Prow == model.Pcol).any()


def test_refusals_leave_the_model_unchanged_and_name_the_place():
    case, dev, model = pair("segments")
    nP = model.length("P")
    for idx, pos in (([0, nP], 1), ([-1, 0], 0), ([0, 1, 0], 2), ([3, 3, 1], 1), ([1, 2, 3, 2, 1], 3)):
        du.expect_refused(dev, model, f"P {idx}", lambda w, idx=idx: w.update_data("P", np.ones(len(idx)), np.array(idx)), pos=pos)
    du.expect_refused(dev, model, "wrong k", lambda w: w.update_data("A", np.ones(model.length("A") - 1)))
    for w in (dev, model):
        w.update_data("P", np.zeros(0))                                  # k = 0: a no-op, not a refusal
        w.update_data("q", np.zeros(0), np.zeros(0, np.int64))
    du.check(dev, model, "no-ops")
    fresh = du.model_of_case(case, *(lambda o: (o.K(), o.maps()))(case_and_oracle("segments")[1]))
    with pytest.raises(du.Refused):
        fresh.update_data("q", np.ones(case.n))                          # before init
    fresh.update_data("P", np.ones(nP))                                  # P and A do not need it
    fresh.deferred = True
    with pytest.raises(du.Refused):
        fresh.update_data("P", np.ones(nP))
