"""PSD cones of side 49 ... 96 on an opted-in handle (hipkkt_kkt_enable_large_psd): the big-class scaling kernel, the
many-workgroup Hs launch and the big-class mul_Hs (k_cone_psd_big, k_psd_hs_big, k_mul_Hs_psd_big), at level B, and K formed
from the device's own scaling at level C (k_psd_A_from_R over psdb_list and the same Hs launch).

Sides: 49 (the smallest new side, odd: it has the dummy pair), 64 (exactly 32 column pairs, the most a 256-thread
workgroup could rotate), 65 and 66 (the first sides past that, odd and even), 96 (the cap), 97 (refused).  Sides up to
66 are checked against the extended-precision reference of tests/cone_reference.py with its own bounds; at side 96,
where that reference costs half a minute, the reference is the CPU oracle and the allowance is 1.25 x bound: the
device's bound plus the quarter that tests/test_large_psd_reference_host.py holds the oracle to."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd.cones import NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT
from tests import cone_reference as cr
from tests.test_gpu_cones import Case, _check, _read, _assert_within

pytestmark = pytest.mark.gpu

BIG_SIDES = (49, 64, 65, 66)
MIXED = [("psd", 49, "interior", 0), ("psd", 48, "interior", 0), ("nn", 7), ("psd", 64, "interior", 0),
         ("psd", 2, "interior", 0), ("soc", 65, None, "both", 3), ("psd", 65, "interior", 0), ("soc", 3, None, "both", 4),
         ("psd", 66, "interior", 0)]
_REF96 = {}


def _is_big(piece):
    return piece[0] == "psd" and piece[1] > 48


def _solver(cones, large=True, P=None, A=None):
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver
    assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
    m = sum(c.numel for c in cones)
    ks = HipKKTSolver(sp.identity(2, format="csc") if P is None else P,
                      sp.csc_matrix(np.ones((m, 2))) if A is None else A, cones)
    if large:
        ks.enable_large_psd()
    return ks


def _run(case, where, factor_may_fail=False):
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(case.s, case.z) or factor_may_fail, where
    out = _read(ks)
    _check(case, ks, out, where)
    return ks, out


# ---- (a) the opt-in and its edges ---------------------------------------------------------------------------------------
def test_opt_in_and_its_edges():
    from cuclarabel_amd import _lib
    case = Case([("psd", 49, "interior", 0)])
    ks = _solver(case.cones, large=False)
    with pytest.raises(_lib.HipKKTError, match="side > 48"):
        ks.kktsolver_update_from_sz(case.s, case.z)
    ks.enable_large_psd(True)
    assert ks.kktsolver_update_from_sz(case.s, case.z) is True
    assert np.all(np.isfinite(ks.mul_Hs(case.z)))
    ks.enable_large_psd(False)
    with pytest.raises(_lib.HipKKTError, match="side > 48"):
        ks.kktsolver_update_from_sz(case.s, case.z)
    with pytest.raises(_lib.HipKKTError, match="needs a device-side scaling"):    # the scaling made while enabled is gone
        ks.mul_Hs(case.z)
    assert _lib.lib().hipkkt_kkt_enable_large_psd(None, 1) == -1                  # HIPKKT_ERR_ARG for a null handle


def test_side_97_is_refused_on_an_enabled_handle_and_nothing_is_written():
    from cuclarabel_amd import _lib
    cones = [NonnegativeConeT(5), PSDTriangleConeT(97)]
    ks = _solver(cones, large=False)
    m = ks.m
    s = np.r_[np.ones(5), cr.svec(np.eye(97))]
    with pytest.raises(_lib.HipKKTError, match="side > 48"):
        ks.kktsolver_update_from_sz(s, s)
    # level B with the caller's Hs fills every block with 7.0; the refused call must leave them alone
    assert ks.kktsolver_update(np.full(ks.info["nHs"], 7.0))
    K0 = ks.KKT().data.copy()
    ks.enable_large_psd(True)
    with pytest.raises(_lib.HipKKTError, match="side > 96"):
        ks.kktsolver_update_from_sz(s, s)
    np.testing.assert_array_equal(ks.get_Hs(), np.full(ks.info["nHs"], 7.0))
    np.testing.assert_array_equal(ks.KKT().data, K0)
    assert m == 5 + 97 * 98 // 2


# ---- (b) scaling parity against the extended-precision reference --------------------------------------------------------
@pytest.mark.parametrize("k", BIG_SIDES)
def test_big_side_alone(k):
    _run(Case([("psd", k, "interior", 0)]), f"PSD({k}) alone")


def test_every_big_side_in_one_handle_beside_small_cones():
    """the work area and the LDS are sized by the largest big side while each cone is laid out by its own k"""
    _run(Case(MIXED, seed=3), "mixed sides")


@pytest.mark.parametrize("cls", ["cond", "late", "cluster"])
def test_spectrum_classes_at_side_65(cls):
    _run(Case([("nn", 5), ("psd", 65, cls, 0), ("soc", 4, None, "both", 0)]), f"PSD(65) {cls}", factor_may_fail=cls == "late")


# ---- (c) side 96 against the oracle -----------------------------------------------------------------------------------------
def _oracle_ref_96():
    """(s, z, reference dictionary from the oracle's lambda, R, Rinv) of one PSD(96), made once for the module"""
    if not _REF96:
        from tests.oracle_bindings import OracleKKT
        k = 96
        s, z = cr.psd_pair(np.random.default_rng(9600), k, "interior")
        o = OracleKKT(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((len(s), 2))), [PSDTriangleConeT(k)])
        assert o.update_scaling(s, z)
        (R, Ri, lam), = o.psd_scaling()
        _REF96.update(s=s, z=z, ref=dict(k=k, lam=lam, R=R, Rinv=Ri, A=R @ R.T, Ainv=Ri.T @ Ri, S=cr.smat(s, k),
                                         Z=cr.smat(z, k)))
    return _REF96["s"], _REF96["z"], _REF96["ref"]


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside-48"])
def test_side_96_against_the_oracle(beside):
    ALLOW = 1.25                   # the device's whole bound plus the oracle's quarter of it
    s96, z96, ref = _oracle_ref_96()
    t = len(s96)
    if beside:
        small = Case([("psd", 48, "interior", 0), ("nn", 3)])
        cones = small.cones + [PSDTriangleConeT(96)]
        s, z = np.r_[small.s, s96], np.r_[small.z, z96]
    else:
        small, cones, s, z = None, [PSDTriangleConeT(96)], s96, z96
    off = len(s) - t
    ks = _solver(cones)
    assert ks.kktsolver_update_from_sz(s, z)
    out = _read(ks)
    R, Ri, lam = out["psd"][-1]
    nh = t * (t + 1) // 2
    Hs = out["Hs"][-nh:]
    rat = cr.psd_ratios(ref, lam, R, Ri, Hs)
    rat["K_Hs"] = cr.ratio(-out["K"][out["maps"]["Hsblocks"][-nh:]] - cr.psd_hs(ref)[0], cr.psd_bounds(ref)["Hs"])
    x = np.random.default_rng(77).standard_normal(len(s))
    yr, yb = cr.psd_mul_Hs(ref, x[off:])
    rat["mulHs"] = cr.ratio(ks.mul_Hs(x)[off:] - yr, yb)
    rat["mulHs_z"] = cr.ratio(ks.mul_Hs(z)[off:] - s96, cr.psd_mul_Hs(ref, z96)[1])
    print(f"PSD(96) {'beside PSD(48)' if beside else 'alone'}: error / bound {rat}")
    bad = {k: v for k, v in rat.items() if not v <= ALLOW}
    assert not bad, f"PSD(96): error / bound > {ALLOW} for {bad}"
    if beside:
        _check(small, ks, dict(out, psd=out["psd"][:-1]), "beside PSD(96)", check_mul=False)


# ---- (d) bit-identity ---------------------------------------------------------------------------------------------------------
def _common_outputs(case, pieces, out, y, keep):
    """the outputs of the cones selected by keep(piece), in order: rows of w / lambda / mul_Hs, eta, Hs blocks and the K
    entries they map to, R and Rinv"""
    rows, wrows, hs, eta, psd, ipsd = [], [], [], [], [], 0
    for ci, (p, c, (off, hoff, *_r)) in enumerate(zip(pieces, case.cones, case.lay)):
        n = c.numel
        nb = n if c.kind in (0, 1) or (c.kind == 2 and c.dim > 4) else n * (n + 1) // 2
        if keep(p):
            rows.append(np.arange(off, off + n))
            if c.kind != 3:                                              # (no kernel writes w on a PSD cone's rows)
                wrows.append(np.arange(off, off + n))
            hs.append(np.arange(hoff, hoff + nb))
            if c.kind == 2:                                              # (eta belongs to second-order cones)
                eta.append(out["eta"][ci])
            if c.kind == 3:
                psd.append(out["psd"][ipsd][:2])
        ipsd += c.kind == 3
    rows, hs = np.concatenate(rows), np.concatenate(hs)
    d = dict(w=out["w"][np.concatenate(wrows)], lam=out["lam"][rows], y=y[rows], eta=np.array(eta), Hs=out["Hs"][hs],
             K=out["K"][out["maps"]["Hsblocks"][hs]])
    for i, (R, Ri) in enumerate(psd):
        d[f"R{i}"], d[f"Rinv{i}"] = R, Ri
    return d


def test_small_cones_and_other_rows_have_the_bits_of_a_twin_without_the_big_cones():
    case = Case(MIXED, seed=3)
    twin_pieces = [p for p in MIXED if not _is_big(p)]
    twin = Case(twin_pieces, seed=3)
    x = np.random.default_rng(5).standard_normal(len(case.s))
    keep_rows = np.concatenate([np.arange(off, off + c.numel) for p, c, (off, *_r) in zip(MIXED, case.cones, case.lay)
                                if not _is_big(p)])
    np.testing.assert_array_equal(case.s[keep_rows], twin.s)
    ka = _solver(case.cones)
    assert ka.kktsolver_update_from_sz(case.s, case.z)
    a = _common_outputs(case, MIXED, _read(ka), ka.mul_Hs(x), lambda p: not _is_big(p))
    kb = _solver(twin.cones, large=False)
    assert kb.kktsolver_update_from_sz(twin.s, twin.z)
    b = _common_outputs(twin, twin_pieces, _read(kb), kb.mul_Hs(x[keep_rows]), lambda p: True)
    assert a.keys() == b.keys()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_an_enabled_handle_without_big_cones_equals_one_never_enabled():
    pieces = [p for p in MIXED if not _is_big(p)]
    case = Case(pieces, seed=3)
    x = np.random.default_rng(5).standard_normal(len(case.s))
    outs = []
    for large in (False, True):
        ks = _solver(case.cones, large=large)
        assert ks.kktsolver_update_from_sz(case.s, case.z)
        o = _read(ks)
        outs.append((o, ks.mul_Hs(x)))
    (o0, y0), (o1, y1) = outs
    not_psd = np.concatenate([np.arange(off, off + c.numel) for c, (off, *_r) in zip(case.cones, case.lay) if c.kind != 3])
    np.testing.assert_array_equal(o0["w"][not_psd], o1["w"][not_psd], err_msg="w")     # (w is not written on PSD rows)
    soc = [i for i, c in enumerate(case.cones) if c.kind == 2]
    np.testing.assert_array_equal(o0["eta"][soc], o1["eta"][soc], err_msg="eta")
    for key in ("lam", "Hs", "K"):
        np.testing.assert_array_equal(o0[key], o1[key], err_msg=key)
    for (R0, Ri0, l0), (R1, Ri1, l1) in zip(o0["psd"], o1["psd"]):
        np.testing.assert_array_equal(R0, R1)
        np.testing.assert_array_equal(Ri0, Ri1)
    np.testing.assert_array_equal(y0, y1)


def test_two_updates_of_the_same_data_agree_bit_for_bit():
    case = Case(MIXED, seed=3)
    ks = _solver(case.cones)
    x = np.random.default_rng(5).standard_normal(len(case.s))
    outs = []
    for _ in range(2):
        assert ks.kktsolver_update_from_sz(case.s, case.z)
        o = _read(ks)
        outs.append((o, ks.mul_Hs(x)))
        assert ks.kktsolver_update_from_sz(case.z, case.s)          # other data in between
    (o0, y0), (o1, y1) = outs
    for key in ("lam", "w", "eta", "Hs", "K"):
        np.testing.assert_array_equal(o0[key], o1[key], err_msg=key)
    for (R0, Ri0, l0), (R1, Ri1, l1) in zip(o0["psd"], o1["psd"]):
        np.testing.assert_array_equal(R0, R1)
        np.testing.assert_array_equal(Ri0, Ri1)
    np.testing.assert_array_equal(y0, y1)


# ---- (e) level C: K from the device's own scaling -------------------------------------------------------------------------
def test_update_scaling_with_the_devices_own_scaling_reproduces_k_exactly():
    """expectation and form of test_gpu_cones.test_level_c_from_the_devices_own_scaling; here the big cones' Hs blocks
    are formed by the same launch from the same R on both routes, so they too must come back bit for bit"""
    from cuclarabel_amd.kktsolver import HipKKTSystem
    case = Case(MIXED, seed=21)
    ka = _solver(case.cones)
    assert ka.kktsolver_update_from_sz(case.s, case.z)
    oa = _read(ka)
    R = np.concatenate([t[0].ravel(order="F") for t in oa["psd"]])
    Ri = np.concatenate([t[1].ravel(order="F") for t in oa["psd"]])
    kb = _solver(case.cones)
    sb = HipKKTSystem(kb)
    sb.init(np.zeros(2), np.zeros(len(case.s)))
    assert sb.update_scaling(oa["w"], oa["eta"], oa["lam"], R, Ri)
    Kb = kb.KKT().data
    mp = oa["maps"]
    small_psd_hs = np.zeros(len(mp["Hsblocks"]), bool)
    for p, c, (off, hoff, *_r) in zip(MIXED, case.cones, case.lay):
        if c.kind == 3 and not _is_big(p):
            small_psd_hs[hoff:hoff + c.numel * (c.numel + 1) // 2] = True
    exact = np.ones(len(Kb), bool)
    exact[mp["Hsblocks"][small_psd_hs]] = False
    np.testing.assert_array_equal(Kb[exact], oa["K"][exact])
    _check(case, kb, dict(oa, K=Kb.copy(), Hs=kb.get_Hs()), "level C mixed", check_mul=False)


@pytest.mark.parametrize("pieces", [[("psd", 64, "interior", 0)], [("nn", 3), ("psd", 65, "interior", 0)]],
                         ids=["psd64", "nn3-psd65"])
def test_a_big_only_list_takes_the_callers_scaling_on_a_fresh_handle(pieces):
    """no PSD cone of side <= 48 in the list: R and Rinv must still reach a handle that has never scaled anything, through
    hipkkt_kkt_system_update_scaling and through hipkkt_kkt_system_update_cones.  K is compared as bits, and a combined-step
    solve (whose right-hand side goes through R: sys_offset, mul_Hs) with the handle that made the scaling."""
    from cuclarabel_amd.kktsolver import HipKKTSystem
    case = Case(pieces, seed=23)
    m = len(case.s)
    rng = np.random.default_rng(31)
    rhs = (rng.standard_normal(2), rng.standard_normal(m), rng.standard_normal(m))
    x = rng.standard_normal(2)

    def system(ks):
        sy = HipKKTSystem(ks)
        sy.init(np.array([0.3, -0.2]), np.linspace(-1.0, 1.0, m))
        return sy

    def step(sy):
        ok, out = sy.solve(rhs[0], rhs[1], rhs[2], 0.7, 0.4, x, case.s, case.z, 1.3, 0.9, False)
        assert ok
        return np.r_[out[0], out[1], out[2], out[3], out[4]]

    ka = _solver(case.cones)
    sa = system(ka)
    assert sa.update(case.s, case.z)
    oa = _read(ka)
    want = step(sa)
    R = np.concatenate([t[0].ravel(order="F") for t in oa["psd"]])
    Ri = np.concatenate([t[1].ravel(order="F") for t in oa["psd"]])
    scale = np.abs(want).max()

    kb = _solver(case.cones)
    sb = system(kb)
    assert sb.update_scaling(oa["w"], oa["eta"], oa["lam"], R, Ri)
    np.testing.assert_array_equal(kb.KKT().data, oa["K"])
    np.testing.assert_array_equal(kb.scaling()[1][0][0], oa["psd"][0][0])
    assert np.abs(step(sb) - want).max() <= 1e-10 * scale

    kc = _solver(case.cones)
    sc = system(kc)
    assert sc.update_cones(oa["Hs"], [], [], [], oa["w"], oa["eta"], oa["lam"], R, Ri)
    np.testing.assert_array_equal(kc.KKT().data, oa["K"])
    np.testing.assert_array_equal(kc.scaling()[1][0][1], oa["psd"][0][1])
    assert np.abs(step(sc) - want).max() <= 1e-10 * scale
    # a missing R is HIPKKT_ERR_ARG, not a silent drop
    from cuclarabel_amd import _lib
    w, eta, lam = (_lib.f64(oa[key]) for key in ("w", "eta", "lam"))
    assert _lib.lib().hipkkt_kkt_system_update_scaling(kc._h, _lib.ptr(w), _lib.ptr(eta), _lib.ptr(lam), None, None) == -1


# ---- (f) a singular S ---------------------------------------------------------------------------------------------------------
def test_a_singular_s_at_side_65_is_reported_without_nan_elsewhere():
    case = Case([("nn", 300), ("soc", 65, None, "both", 1), ("psd", 8, "interior", 0), ("psd", 65, "interior", 0)], seed=6)
    s = case.s.copy()
    off = case.lay[3][0]
    G = np.random.default_rng(1).standard_normal((65, 65))
    S = G @ G.T / 65 + np.eye(65)
    S[-1, :] = S[:, -1] = 0.0                                        # singular: the last Cholesky pivot is exactly 0
    s[off:off + 65 * 66 // 2] = cr.svec(S)
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(s, case.z) is False
    out = _read(ks)
    assert np.all(np.isfinite(out["w"][:off])) and np.all(np.isfinite(out["lam"][:off]))
    np.testing.assert_array_equal(out["w"][:300], np.sqrt(case.s[:300] / case.z[:300]))
    sl = slice(case.lay[1][0], case.lay[1][0] + 65)
    _assert_within(cr.soc_ratios(case.refs[1][1], lam=out["lam"][sl], w=out["w"][sl]), "SOC next to a singular PSD(65)")
    R, Ri, lam = out["psd"][0]
    hoff = case.lay[2][1]
    _assert_within(cr.psd_ratios(case.refs[2][1], lam, R, Ri, out["Hs"][hoff:hoff + 36 * 37 // 2]), "PSD(8) next to it")


# ---- (g) level B solve with the device's own scaling ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [49, 65])
def test_level_b_solve_with_the_devices_own_scaling(k):
    from tests.oracle_bindings import OracleKKT
    cones = [NonnegativeConeT(4), PSDTriangleConeT(k), SecondOrderConeT(6)]
    rng = np.random.default_rng(k)
    m = sum(c.numel for c in cones)
    A = sp.random(m, 30, density=0.05, random_state=rng, data_rvs=rng.standard_normal).tocsc()
    P = sp.identity(30, format="csc")
    sk, zk = cr.psd_pair(rng, k)
    s6, z6 = cr.soc_pair(rng, 6)
    s = np.r_[cr.nn_point(rng, 4), sk, s6]
    z = np.r_[cr.nn_point(rng, 4), zk, z6]
    ks = _solver(cones, P=P, A=A)
    o = OracleKKT(P, A, cones, perm=ks.perm())
    assert o.update_scaling(s, z) and o.kktsolver_update()
    assert ks.kktsolver_update_from_sz(s, z)
    rx, rz = rng.standard_normal(30), rng.standard_normal(m)
    ks.kktsolver_setrhs(rx, rz)
    x, zz = np.zeros(30), np.zeros(m)
    assert ks.kktsolver_solve(x, zz)
    o.kktsolver_setrhs(rx, rz)
    ok, xo, zo = o.kktsolver_solve()
    assert ok
    scale = max(np.abs(xo).max(), np.abs(zo).max())
    assert max(np.abs(x - xo).max(), np.abs(zz - zo).max()) <= 1e-9 * scale
