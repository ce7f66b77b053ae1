"""The KKT value path on the device against tests/kvalue_reference.py: what k_scatter, k_update_values (three index
segments in one launch, written through to the residual's copy), k_gather_values and the regulariser's reduction put into
K's two copies, after every step of sequences that take every branch of the protocol between them (fval_dirty, gather,
write-through, suppressed write-through), at the edges of the launches: segment boundaries on workgroup edges, the
`total % 256` tail, the grid-stride second trips past 4096 x 256 items, the reduction past 256 x 256 rows.

After every step:  ks.KKT().data is the model's Kval byte for byte;  the image the residual reads -- probed exactly with
columns of the identity, where ks.residual(X, 0) returns -K[:, j] with one product by 1.0 per entry -- equals the image
of those values;  after a cone update the regulariser equals the model's with ==.  Handles too large for N / 64 probe
calls are probed with two random columns against the exact residual and its order-free bound, with every step's values
a factor outside [0.5, 2] away from the ones they replace (asserted on the inputs).

Where the model cannot predict the values bit for bit (scalings computed on the device), the image is compared with the
image of the handle's own KKT().data: the two copies must agree whatever they hold."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from tests import kvalue_reference as kv

pytestmark = pytest.mark.gpu

_H, _T = {}, {}


def _case(name):
    if name == "psd_wrap":
        return kv.case_psd_wrap()
    if name == "banded_big":
        return kv.case_banded_big()
    return kv.SMALL_CASES[name]()


def new_handle(case, **settings):
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver
    ks = HipKKTSolver(case.P, case.A, case.cones, settings=_lib.default_settings(**settings) if settings else None)
    return ks, kv.model_of_handle(ks, case.P, case.A)


def handle(name):
    """(case, ks, model) per module: creation is the cost.  The model has received every call the handle has."""
    if name not in _H:
        case = _case(name)
        t0 = time.perf_counter()
        ks, model = new_handle(case)
        _T[name] = time.perf_counter() - t0
        print(f"\n[kkt values] {name}: N {ks.N} nnzK {ks.info['nnzK']} nHs {ks.info['nHs']} created in {_T[name]:.2f} s")
        assert model.c0 == kv.REG_C0 and model.c1 == kv.REG_C1 and model.reg_enable
        _H[name] = (case, ks, model)
    return _H[name]


def teardown_module():
    _H.clear()                                               # (the handles go while the library is still loaded)


LEVEL_B = ["segments"] + [f"block_edge[{nn},{k}]" for nn, k in kv.BLOCK_EDGES] + ["many_soc", "psd_wrap"]


def assert_counts(name, ks, model):
    """the count each case is named after, from the handle: an error, never a skip"""
    i = ks.info
    assert (i["nHs"], i["sparse_soc_len"], i["nsparse_soc"]) == (model.nHs, model.sparse_len, model.nsparse)
    if name == "segments":
        assert (i["nHs"], i["sparse_soc_len"], i["nsparse_soc"]) == (33, 12, 2) and model.total <= 64
    elif name.startswith("block_edge"):
        nn, k = (int(t) for t in name[len("block_edge["):-1].split(","))
        assert (i["nHs"], i["sparse_soc_len"], i["nsparse_soc"]) == (nn + k, k, 1)
        assert i["nHs"] in (255, 256, 257) or i["nHs"] + i["sparse_soc_len"] in (255, 256, 257)
        assert model.total % 256 == (nn + 2 * k + 1) % 256
    elif name == "many_soc":
        assert (i["nHs"], i["sparse_soc_len"], i["nsparse_soc"]) == (1500, 1500, 300)
        assert 3000 // 256 < (model.total - 1) // 256
    elif name == "psd_wrap":
        assert i["nHs"] == 2 * 692_076 + 8 > kv.UPDATE_GRID_CAP * kv.UPDATE_BLOCK == 2 ** 20
        assert model.vmap.size > 2 ** 21 and i["N"] == 2376 <= kv.EXACT_PROBE_MAX_N
    elif name == "banded_big":
        assert model.maps["A"].size == 1_048_580 > 2 ** 20 and i["N"] == 419_432 > kv.RED_BLOCKS * kv.UPDATE_BLOCK == 65_536
        assert model.vmap.size > 2 ** 21


# ------------------------------------------------------------------------------------------------ level B, host route
@pytest.mark.parametrize("name", LEVEL_B)
def test_level_b_sequences_1_to_6(name):
    """create | update | update, solve, update | update_P | update_A, update | update: values, image and regulariser
    after each (kvalue_reference.sequence_level_b)."""
    case, ks, model = handle(name)
    assert_counts(name, ks, model)
    kv.sequence_level_b(ks, model, case)
    assert ks.fallbacks == (0, 0)


@pytest.mark.parametrize("name", LEVEL_B)
def test_sequence_7_first_update_on_a_never_probed_handle(name):
    case = _case(name)
    ks, model = new_handle(case)
    kv.sequence_fresh(ks, model, case)


def test_banded_big_second_trips_of_scatter_gather_and_reduction():
    """nnzA = 1 048 580: k_scatter's second trip in update_A; an image of 2.5 M entries: k_gather_values' second trip;
    N = 419 432: k_diag_absmax strides.  update(H1), update_A(A2), update(H2), update(H3) with the bounded probe after
    each: the first probe gathers, update(H2) is suppressed behind update_A, update(H3) writes through."""
    case = _case("banded_big")                                # a handle of its own: the sequence starts from creation
    t0 = time.perf_counter()
    ks, model = new_handle(case)
    created = time.perf_counter() - t0
    assert_counts("banded_big", ks, model)
    t0 = time.perf_counter()
    kv._update(ks, model, case, 0, "big update(H1)")
    kv._check(ks, model, "big update(H1)", eps=True, seed=10)
    A2 = case.A2()
    kv.assert_changed(case.A.data, A2, "big A2")
    ks.kktsolver_update_A(A2)
    model.update_A(A2)
    kv._update(ks, model, case, 1, "big update(H2)")
    kv._check(ks, model, "big update_A update(H2)", eps=True, seed=11)
    kv._update(ks, model, case, 2, "big update(H3)")
    kv._check(ks, model, "big update(H3) write-through", eps=True, seed=12)
    print(f"\n[kkt values] banded_big: created in {created:.2f} s (with its model), sequence in {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------ scalings from (s, z)
def _interior(cones, seed):
    from cuclarabel_amd import problems
    return problems.interior_point(cones, np.random.default_rng(seed))


def assert_coherent(ks, model, tag, seed=0):
    """the two copies agree, whatever they hold; -> K values"""
    vals = ks.KKT().data
    assert np.isfinite(vals).all(), tag
    kv.assert_image(ks, model, tag, Kval=vals, seed=seed)
    return vals


def assert_device_scaled_values(ks, model, vals, tag):
    m = model.maps
    assert np.array_equal(vals[m["Hsblocks"]], -ks.get_Hs()), tag
    assert np.array_equal(vals[m["soc_D"][0::2]], -vals[m["soc_D"][1::2]]), tag
    assert (vals[m["soc_D"][1::2]] > 0).all(), tag


@pytest.mark.parametrize("name", ["segments", "many_soc"])
def test_sequence_8_update_from_sz_twice(name):
    case = _case(name)
    ks, model = new_handle(case)
    kv.assert_image(ks, model, f"{name} create")                          # the copy is current: write-through from here on
    old = None
    for it in range(2):
        s, z = _interior(case.cones, 900 + it), _interior(case.cones, 950 + it)
        assert ks.kktsolver_update_from_sz(s, z)
        vals = assert_coherent(ks, model, f"{name} update_from_sz #{it + 1}")
        assert_device_scaled_values(ks, model, vals, f"{name} update_from_sz #{it + 1}")
        assert old is None or not np.array_equal(vals[model.maps["Hsblocks"]], old[model.maps["Hsblocks"]])
        old = vals


def test_deferred_status_updates_write_through():
    """hipkkt_kkt_set_deferred_status: two enqueue-only updates from device tensors, then the probe"""
    import torch
    case = _case("segments")
    ks, model = new_handle(case)
    kv.assert_image(ks, model, "deferred create")
    dev = torch.device("cuda")
    pairs = [(torch.from_numpy(_interior(case.cones, 910 + i)).to(dev), torch.from_numpy(_interior(case.cones, 960 + i)).to(dev))
             for i in range(2)]
    torch.cuda.synchronize()
    ks.set_deferred_status(True)
    try:
        for ds, dz in pairs:
            assert ks.kktsolver_update_from_sz_dev(ds.data_ptr(), dz.data_ptr())
        vals = assert_coherent(ks, model, "deferred update x 2")
        assert_device_scaled_values(ks, model, vals, "deferred update x 2")
        assert ks.deferred_status() == 0
    finally:
        ks.set_deferred_status(False)
    ref, _ = new_handle(case)                                             # the synchronous call leaves the same values
    assert ref.kktsolver_update_from_sz(pairs[1][0].cpu().numpy(), pairs[1][1].cpu().numpy())
    assert ref.KKT().data.tobytes() == vals.tobytes()


# ------------------------------------------------------------------------------------------------ generalized power cones
def genpow_problem():
    """zero, nonnegative, sparse second-order, exponential and power cones, a generalized power cone on one wave (4 rows)
    and one on a workgroup (700 rows > 512); P = A = I"""
    from cuclarabel_amd import problems
    from cuclarabel_amd.cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, ExponentialConeT, PowerConeT, GenPowerConeT)
    cones = [ZeroConeT(2), NonnegativeConeT(3), SecondOrderConeT(6), ExponentialConeT(), PowerConeT(0.4),
             GenPowerConeT([0.4, 0.6], 2), GenPowerConeT(problems.normalised_alphas(np.linspace(0.5, 1.5, 300)), 400)]
    m = sum(c.numel for c in cones)
    assert min(c.numel for c in cones if c.kind == 6) <= 512 < max(c.numel for c in cones if c.kind == 6)
    return sp.identity(m, format="csc"), sp.identity(m, format="csc"), cones


def genpow_pair(cones, seed):
    """(s, z) strictly inside the cones and their duals"""
    from tests import genpow_reference as gr
    from tests import nonsymmetric_reference as nr
    rng = np.random.default_rng(seed)
    s, z = [], []
    for c in cones:
        if c.kind == 0:
            a, b = np.zeros(c.numel), rng.standard_normal(c.numel)
        elif c.kind == 1:
            a, b = np.exp(rng.standard_normal(c.numel)), np.exp(rng.standard_normal(c.numel))
        elif c.kind == 2:
            a, b = rng.standard_normal(c.numel), rng.standard_normal(c.numel)
            a[0], b[0] = np.linalg.norm(a[1:]) + 1.0, np.linalg.norm(b[1:]) + 1.0
        elif c.kind == 6:
            a, b = gr.random_interior_pair(c, rng)
        else:
            a, b = nr.random_interior_pair(c, rng)
        s.append(a)
        z.append(b)
    return np.concatenate(s), np.concatenate(z)


def assert_genpow_values(ks, model, vals, tag):
    assert_device_scaled_values(ks, model, vals, tag)
    D = vals[ks.maps()["genpow_D"]].reshape(-1, 3)
    assert D.shape[0] == 2 and np.array_equal(D, np.tile([-1.0, -1.0, 1.0], (2, 1))), (tag, D)


def genpow_handle():
    from cuclarabel_amd import ipm
    from cuclarabel_amd.kktsolver import HipKKTSolver
    P, A, cones = genpow_problem()
    ks = HipKKTSolver(P, A, cones)
    ks.set_nonsymmetric_scaling(ipm.DUAL, 0.7)
    K = ks.KKT()
    model = kv.KModel(K.indptr, K.indices, {k: v for k, v in ks.maps().items() if not k.startswith("genpow")}, cones, P.data, A.data)
    assert ks.N <= kv.EXACT_PROBE_MAX_N
    return P, A, cones, ks, model


def test_sequence_8_on_generalized_power_cones():
    """update_from_sz only: the scaling kernel of the generalized power cones writes p, q, r and D through put_k as well"""
    P, A, cones, ks, model = genpow_handle()
    kv.assert_values(ks, model, "genpow create")
    kv.assert_image(ks, model, "genpow create")
    old = None
    for it in range(2):
        s, z = genpow_pair(cones, 1200 + it)
        assert ks.kktsolver_update_from_sz(s, z)
        vals = assert_coherent(ks, model, f"genpow update_from_sz #{it + 1}")
        assert_genpow_values(ks, model, vals, f"genpow update_from_sz #{it + 1}")
        gp = ks.maps()["genpow_p"]
        assert (vals[gp] != 0).all() and (old is None or (vals[gp] != old[gp]).all())
        old = vals


# ------------------------------------------------------------------------------------------------ level C
@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("name", ["segments", "genpow"])
def test_level_c_updates_keep_the_copies_coherent(name, lazy):
    """HipKKTSystem.update_dev twice (in lazy mode the second is only enqueued), update_P, update_dev"""
    import torch
    from cuclarabel_amd.kktsolver import HipKKTSystem
    if name == "genpow":
        P, A, cones, ks, model = genpow_handle()
        pairs = [genpow_pair(cones, 1300 + i) for i in range(3)]
        check = assert_genpow_values
    else:
        case = _case(name)
        P, A, cones = case.P, case.A, case.cones
        ks, model = new_handle(case)
        pairs = [(_interior(cones, 1400 + i), _interior(cones, 1450 + i)) for i in range(3)]
        check = assert_device_scaled_values
    system = HipKKTSystem(ks)
    rng = np.random.default_rng(31)
    system.init(rng.standard_normal(ks.n), rng.standard_normal(ks.m))
    if lazy:
        system.set_lazy(True)
    dev = torch.device("cuda")
    d = [(torch.from_numpy(s).to(dev), torch.from_numpy(z).to(dev)) for s, z in pairs]
    torch.cuda.synchronize()
    kv.assert_image(ks, model, f"{name} create", Kval=ks.KKT().data)
    for i in range(2):
        assert system.update_dev(d[i][0].data_ptr(), d[i][1].data_ptr())
        check(ks, model, assert_coherent(ks, model, f"{name} level C update #{i + 1}"), f"{name} level C update #{i + 1}")
    P2 = sp.csc_matrix(P).copy()
    P2.data = P2.data * np.where(np.arange(P2.nnz) % 2 == 0, 4.0, 0.125)
    ks.kktsolver_update_P(P2)
    vals = assert_coherent(ks, model, f"{name} level C update_P")
    assert np.array_equal(vals[model.maps["P"]], P2.data)
    assert system.update_dev(d[2][0].data_ptr(), d[2][1].data_ptr())
    vals = assert_coherent(ks, model, f"{name} level C update after update_P")
    check(ks, model, vals, f"{name} level C update after update_P")
    assert np.array_equal(vals[model.maps["P"]], P2.data)
    if lazy:
        assert system.set_lazy(False)                                       # the enqueued updates' status and the solve that was due
    assert ks.fallbacks == (0, 0)


def hs_rows_of_psd(cones):
    """which entries of the Hs blocks belong to PSD cones (blocks in cone order: packed triangles for dense cones)"""
    from cuclarabel_amd.cones import SOC_NO_EXPANSION_MAX_SIZE
    out = []
    for c in cones:
        dense = c.kind == 3 or (c.kind == 2 and c.dim <= SOC_NO_EXPANSION_MAX_SIZE)
        out.append(np.full(c.numel * (c.numel + 1) // 2 if dense else c.numel, c.kind == 3))
    return np.concatenate(out)


def test_update_scaling_from_a_read_back_scaling():
    """hipkkt_kkt_system_update_scaling on a second handle, from the first handle's (w, eta, lambda, R, Rinv): Hs, u, v and
    eta^2 are formed on the device from the scaling and go through the same k_update_values.  Its K equals the first
    handle's byte for byte -- u, v and D entries included -- except the Hs block of the PSD cone, which update_scaling
    forms from R R' and update_from_sz from the factorisation behind R (not bit-identical; tests/test_gpu_cones.py makes
    the same exception).  Every Hs entry outside that block is therefore what update_cones writes from the FIRST
    handle's get_Hs(): the negated copy.  The second call writes through; the copies are coherent after both."""
    from cuclarabel_amd.kktsolver import HipKKTSystem
    case = _case("segments")
    first, model = new_handle(case)
    s, z = _interior(case.cones, 1500), _interior(case.cones, 1550)
    assert first.kktsolver_update_from_sz(s, z)
    K1, Hs1 = first.KKT().data, first.get_Hs()
    w, eta = first.scaling_w()
    lam, psd = first.scaling()
    R = np.concatenate([r.ravel(order="F") for r, _, _ in psd] + [np.zeros(0)])
    Ri = np.concatenate([ri.ravel(order="F") for _, ri, _ in psd] + [np.zeros(0)])
    second, _ = new_handle(case)
    system = HipKKTSystem(second)
    rng = np.random.default_rng(32)
    system.init(rng.standard_normal(second.n), rng.standard_normal(second.m))
    kv.assert_image(second, model, "update_scaling create")
    psd_hs = hs_rows_of_psd(case.cones)
    assert psd_hs.size == model.nHs and psd_hs.sum() == 6
    same = np.ones(K1.size, bool)
    same[model.maps["Hsblocks"][psd_hs]] = False
    for it in range(2):                                                   # the second call writes through
        assert system.update_scaling(w, eta, lam, R, Ri)
        vals = assert_coherent(second, model, f"update_scaling #{it + 1}")
        assert_device_scaled_values(second, model, vals, f"update_scaling #{it + 1}")
        assert vals[same].tobytes() == K1[same].tobytes(), f"update_scaling #{it + 1}"
        assert vals[model.maps["Hsblocks"][~psd_hs]].tobytes() == (-Hs1[~psd_hs]).tobytes()
        assert (vals[model.maps["soc_u"]] != 0).all() and (vals[model.maps["soc_v"]][1:] != 0).any()


# ------------------------------------------------------------------------------------------------ the regulariser
PLACEMENTS = [("segments", p) for p in ("0", "N-1", "-Hs", "+eta2")] + \
             [("block_edge[246,10]", p) for p in ("0", "255", "256", "N-1", "-Hs", "+eta2")] + \
             [("banded_big", p) for p in ("0", "255", "256", "N-1", "65536+300", "-Hs")]


@pytest.mark.parametrize("name,where", PLACEMENTS, ids=lambda v: str(v))
def test_regulariser_finds_the_maximum_wherever_it_sits(name, where):
    """2^40 at one diagonal position, positive values of order one elsewhere, through the host route: eps is
    c0 + c1 2^40 bit for bit, and differs from what the second largest entry would give."""
    if name == "banded_big":
        case, ks, model = handle(name)                        # (shared by the placements alone; each sets every value it reads)
        assert_counts(name, ks, model)
    else:
        case = _case(name)
        ks, model = new_handle(case)
    pos = kv.placement_positions(model, big=(name == "banded_big"))
    if where in ("255", "256") and where not in pos:
        pytest.fail(f"{name} has no diagonal position {where}")
    kv.run_placement(ks, model, case, where, pos[where])


def test_regulariser_with_a_proportional_part_that_rounds():
    """c1 = 1e-3 (no power of two): the product and the sum each round once"""
    case = _case("segments")
    ks, model = new_handle(case, static_regularization_proportional=1e-3)
    assert model.c1 == 1e-3
    for step in range(2):
        kv._update(ks, model, case, step, f"c1=1e-3 update #{step + 1}")
        kv.assert_eps(ks, model, f"c1=1e-3 update #{step + 1}")
        d = np.abs(model.Kval[model.maps["diag_full"]]).max()
        assert model.eps == kv.REG_C0 + 1e-3 * d and model.eps > kv.REG_C0


def test_regulariser_switched_off_and_constant_only():
    case = _case("block_edge[246,10]")                      # (no zero cone: quasi-definite without a regulariser)
    ks, model = new_handle(case, static_regularization_enable=0)
    kv._update(ks, model, case, 0, "reg off")
    assert ks.diagonal_regularizer == 0.0 == model.eps
    kv.assert_values(ks, model, "reg off")
    case = _case("segments")
    ks, model = new_handle(case, static_regularization_proportional=0.0)
    kv._update(ks, model, case, 0, "c1=0")
    assert ks.diagonal_regularizer == kv.REG_C0 == model.eps
