"""The host model of K's two copies (tests/kvalue_reference.py) and the design of the sequences that
tests/test_gpu_kkt_values.py runs on the device -- no GPU.  The pattern and the maps are the oracle's, which
test_assembly_maps_bit_exact pins as equal to the library's.

  - every sequence on a fault-free model passes the three helpers;
  - every seeded fault makes the helper that should see it raise, in a sequence named here;
  - kpos, the image order and expected_image() agree with residual_reference.sym_from_triu on the oracle's K."""
import numpy as np
import pytest

from tests import kvalue_reference as kv
from tests import residual_reference as rr
from tests.oracle_bindings import OracleKKT

_CASES = {}


def case_and_oracle(name):
    if name not in _CASES:
        case = kv.SMALL_CASES[name]()
        _CASES[name] = (case, OracleKKT(case.P, case.A, case.cones))
    return _CASES[name]


def pair(name, fault=None):
    """(device, model): a model with the fault standing in for the handle, and the fault-free one"""
    case, o = case_and_oracle(name)
    return case, kv.model_of_oracle(o, case.P, case.A, case.cones, fault=fault), kv.model_of_oracle(o, case.P, case.A, case.cones)


@pytest.mark.parametrize("name", sorted(kv.SMALL_CASES))
def test_case_counts_are_what_the_cases_are_named_after(name):
    case, o = case_and_oracle(name)
    model = kv.model_of_oracle(o, case.P, case.A, case.cones)
    if name == "segments":
        assert (model.nHs, model.sparse_len, model.nsparse) == (33, 12, 2) and model.total < 64
        e2 = case.hs(0)[3]
        assert e2[0] != e2[1]
    elif name == "many_soc":
        assert (model.nHs, model.sparse_len, model.nsparse) == (1500, 1500, 300)
        assert (model.nHs + model.sparse_len) // 256 < (model.total - 1) // 256      # the D segment spans a workgroup edge
    else:
        nn, k = case.cones[0].dim, case.cones[1].dim
        assert (model.nHs, model.sparse_len, model.nsparse) == (nn + k, k, 1)
        assert model.total % 256 == (nn + 2 * k + 1) % 256
    assert model.N == o.N and model.nnzK == o.nnzK


def test_block_edge_boundaries_sit_before_on_and_after_a_workgroup_edge():
    nhs = [nn + k for nn, k in kv.BLOCK_EDGES[:3]]
    assert nhs == [255, 256, 257]
    ends = [nn + 2 * k for nn, k in (kv.BLOCK_EDGES[3], kv.BLOCK_EDGES[1], kv.BLOCK_EDGES[4])]
    assert ends == [264, 266, 268]
    assert [nn + 2 * k for nn, k in kv.BLOCK_EDGES[5:]] == [255, 256, 257]          # the sparse / D boundary itself
    tails = [(nn + 2 * k + 1) % 256 for nn, k in kv.BLOCK_EDGES]
    assert tails[5:] == [0, 1, 2]
    assert len(set(tails[:3])) == 3 and len({tails[3], tails[1], tails[4]}) == 3


@pytest.mark.parametrize("name", sorted(kv.SMALL_CASES))
def test_fault_free_model_passes_every_sequence(name):
    case, dev, model = pair(name)
    kv.sequence_level_b(dev, model, case)
    case, dev, model = pair(name)
    kv.sequence_fresh(dev, model, case)


@pytest.mark.parametrize("name", ["segments", "block_edge[246,10]"])
def test_fault_free_model_passes_every_placement(name):
    case, dev, model = pair(name)
    pos = kv.placement_positions(model)
    assert {"0", "N-1", "-Hs", "+eta2"} <= set(pos) and (name == "segments" or {"255", "256"} <= set(pos))
    for label, p in pos.items():
        kv.run_placement(dev, model, case, label, p)


# fault -> (case, sequence, the step and the helper that must raise)
EXPOSED_BY = {
    "second_slot": ("segments", "level_b", "assert_image", "seq2"),              # the first write-through
    "through_while_dirty": ("segments", "level_b", "assert_image", "seq5"),      # a cone update behind update_A
    "P_not_dirty": ("segments", "level_b", "assert_image", "seq4"),              # update_P, then the probe must gather
    "cone_lookup": ("segments", "level_b", "assert_values", "seq2"),             # two sparse cones, different eta^2
    "D_signs": ("segments", "level_b", "assert_values", "seq2"),
    "tail_skipped": ("block_edge[246,10]", "level_b", "assert_values", "seq2"),  # total = 267: the last 11 items
    "last_partial": ("block_edge[246,10]", "placement N-1", "assert_eps", "N-1"),  # N = 266: two partials, the maximum in the last
}


@pytest.mark.parametrize("fault", kv.FAULTS)
def test_every_seeded_fault_is_seen_by_a_named_sequence(fault):
    name, seq, helper, step = EXPOSED_BY[fault]
    case, dev, model = pair(name, fault)
    with pytest.raises(kv.ValuePathError) as err:
        if seq == "level_b":
            kv.sequence_level_b(dev, model, case)
        else:
            kv.run_placement(dev, model, case, "N-1", kv.placement_positions(model)["N-1"])
    assert err.value.helper == helper and step in str(err.value), str(err.value)


def test_fresh_sequence_sees_a_write_through_into_a_never_gathered_copy():
    """sequence 7 is the only one whose first update meets a copy that was never gathered"""
    case, dev, model = pair("segments", "through_while_dirty")
    with pytest.raises(kv.ValuePathError) as err:
        kv.sequence_fresh(dev, model, case)
    assert err.value.helper == "assert_image"


def test_last_partial_fault_is_invisible_where_the_maximum_sits_elsewhere():
    """the placement cases are needed: with the maximum at position 0 the fault passes"""
    case, dev, model = pair("block_edge[246,10]", "last_partial")
    kv.run_placement(dev, model, case, "0", 0)


@pytest.mark.parametrize("name", ["segments", "block_edge[245,10]", "many_soc"])
def test_image_order_kpos_and_expected_image_agree_with_sym_from_triu(name):
    case, o = case_and_oracle(name)
    model = kv.model_of_oracle(o, case.P, case.A, case.cones)
    K = o.K()
    rng = np.random.default_rng(3)
    vals = rng.standard_normal(K.nnz)
    ref = rr.sym_from_triu(K.indptr, K.indices, vals)
    assert np.array_equal(model.indptr, ref.indptr) and np.array_equal(model.indices, ref.indices)
    assert np.array_equal(vals[model.vmap], ref.data)
    img = model.expected_image(vals)
    assert np.array_equal(img.data, ref.data) and np.array_equal(img.indices, ref.indices)
    # kpos as the library's loop builds it: first free slot, then second
    kp = np.full(2 * K.nnz, -1, dtype=np.int64)
    for q, e in enumerate(model.vmap):
        if kp[2 * e] < 0:
            kp[2 * e] = q
        else:
            kp[2 * e + 1] = q
    assert np.array_equal(model.kpos, kp)
    col = np.repeat(np.arange(model.N), np.diff(model.colptr))
    diag = model.rowval == col
    assert (model.kpos[1::2][diag] == -1).all() and (model.kpos[1::2][~diag] > model.kpos[0::2][~diag]).all()
    assert (model.kpos[0::2] >= 0).all()
    # the oracle's K right after creation is the model's: P and A copied, zero elsewhere
    assert np.array_equal(K.data, model.Kval)
    assert np.array_equal(model.maps["diag_full"], model.colptr[1:] - 1)


def test_model_values_are_the_oracles_after_an_update():
    """the model's arithmetic against the oracle's update of the same (Hs, u, v, eta^2): K values and regulariser"""
    case, o = case_and_oracle("segments")
    model = kv.model_of_oracle(o, case.P, case.A, case.cones)
    Hs, u, v, e2 = case.hs(0)
    model.update_cones(Hs, u, v, e2)
    assert o.kktsolver_update_values(Hs, u, v, e2)
    assert np.array_equal(o.K().data, model.Kval)
    assert o.last_regularizer == model.eps


def test_regulariser_settings():
    case, o = case_and_oracle("segments")
    Hs, u, v, e2 = case.hs(0)
    off = kv.model_of_oracle(o, case.P, case.A, case.cones, reg_enable=False)
    off.update_cones(Hs, u, v, e2)
    assert off.eps == 0.0
    const = kv.model_of_oracle(o, case.P, case.A, case.cones, c1=0.0)
    const.update_cones(Hs, u, v, e2)
    assert const.eps == kv.REG_C0


def test_assert_changed_rejects_a_value_within_a_factor_two():
    kv.assert_changed([1.0, 0.0, 0.0, -2.0], [2.5, 0.0, 1.0, -0.9])
    with pytest.raises(AssertionError):
        kv.assert_changed([1.0], [1.9])
