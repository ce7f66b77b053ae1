"""The device cone scalings (k_cone_scaling, k_cone_psd, k_mul_Hs, k_mul_Hs_psd and the level-C kernels that form K's
values from a caller's scaling) against the extended-precision reference of tests/cone_reference.py, at the shapes
where the kernels could go wrong: every PSD side class up to the LDS limit of 48 (odd sides, mixed sides in one handle),
second-order cones at wave-stride edges and near the cone boundary, elementwise grids that end next to the SOC
workgroups, exact power-of-two scalings (outputs must scale exactly) and scale extremes.  Worst error / bound per
quantity is printed under -s."""
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd.cones import ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT
from tests import cone_reference as cr

pytestmark = pytest.mark.gpu

PSD_SIDES = (1, 2, 3, 7, 8, 15, 16, 17, 24, 25, 31, 32, 33, 40, 47, 48)
WORST = cr.Worst("device cone scalings against the extended-precision reference")
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    WORST.report()


def _assert_within(ratios, where):
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{where}: error / bound > 1 for {bad}"


def _solver(cones):
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver
    assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
    m = sum(c.numel for c in cones)
    return HipKKTSolver(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((m, 2))), cones)


def _psd(k, cls="interior", seed=0):
    """(s, z, reference) of one PSD cone, cached for the module (the reference costs seconds at side 48)"""
    key = ("psd", k, cls, seed)
    if key not in _REF:
        s, z = cr.psd_pair(np.random.default_rng(10_000 * seed + 100 * k + cr.PSD_CLASSES.index(cls)), k, cls)
        _REF[key] = (s, z, cr.psd_ref(s, z, k))
    return _REF[key]


def _soc(n, delta=None, which="both", seed=0):
    key = ("soc", n, delta, which, seed)
    if key not in _REF:
        s, z = cr.soc_pair(np.random.default_rng(zlib.crc32(repr(key).encode())), n, delta, which)
        _REF[key] = (s, z, cr.soc_ref(s, z))
    return _REF[key]


def _layout(cones):
    """per cone: (off in m, offset of its Hs block, index among sparse SOCs or -1, offset in the sparse u/v arrays)"""
    out, off, hoff, sidx, soff = [], 0, 0, 0, 0
    for c in cones:
        n = c.numel
        if c.kind == 2 and c.dim > 4:
            out.append((off, hoff, sidx, soff))
            sidx += 1
            soff += n
            hoff += n
        else:
            out.append((off, hoff, -1, -1))
            hoff += n * (n + 1) // 2 if c.kind in (2, 3) else n
        off += n
    return out


class Case:
    """a cone list with its (s, z) and references; pieces: ('nn', n) | ('zero', n) | ('soc', n, delta, which, seed) |
    ('psd', k, cls, seed)"""

    def __init__(self, pieces, seed=1):
        rng = np.random.default_rng(seed)
        self.cones, ss, zz, self.refs = [], [], [], []
        for p in pieces:
            if p[0] == "nn":
                s, z = cr.nn_point(rng, p[1]), cr.nn_point(rng, p[1])
                self.cones.append(NonnegativeConeT(p[1]))
                ref = ("nn", None)
            elif p[0] == "zero":
                s, z = np.zeros(p[1]), cr.nn_point(rng, p[1])
                self.cones.append(ZeroConeT(p[1]))
                ref = ("zero", None)
            elif p[0] == "soc":
                s, z, r = _soc(*p[1:])
                self.cones.append(SecondOrderConeT(p[1]))
                ref = ("soc", r)
            else:
                s, z, r = _psd(*p[1:])
                self.cones.append(PSDTriangleConeT(p[1]))
                ref = ("psd", r)
            ss.append(s)
            zz.append(z)
            self.refs.append(ref)
        self.s, self.z = np.concatenate(ss), np.concatenate(zz)
        self.lay = _layout(self.cones)


def _read(ks):
    lam, psd = ks.scaling()
    w, eta = ks.scaling_w()
    return dict(lam=lam, psd=psd, w=w, eta=eta, Hs=ks.get_Hs(), K=ks.KKT().data.copy(), maps=ks.maps())


def _check(case, ks, out, where, scale=(0, 0), check_mul=True):
    """every cone's outputs against the reference (scaled by 2^a, 2^b when the inputs were)"""
    a, b = scale
    fs, fz = 2.0 ** a, 2.0 ** b
    mp = out["maps"]
    Kd = out["K"]
    x = np.random.default_rng(77).standard_normal(len(case.s))
    y = ks.mul_Hs(x) if check_mul else None
    yz = ks.mul_Hs(case.z * fz) if check_mul else None
    ipsd = 0
    for ci, (c, (kind, ref), (off, hoff, sidx, soff)) in enumerate(zip(case.cones, case.refs, case.lay)):
        n = c.numel
        sl = slice(off, off + n)
        if kind in ("nn", "zero"):
            s, z = case.s[sl] * fs, case.z[sl] * fz
            w = np.sqrt(s / z) if kind == "nn" else np.zeros(n)
            np.testing.assert_array_equal(out["w"][sl], w, err_msg=where)
            np.testing.assert_array_equal(out["Hs"][hoff:hoff + n], w * w, err_msg=where)
            np.testing.assert_array_equal(Kd[mp["Hsblocks"][hoff:hoff + n]], -(w * w), err_msg=where)
            if check_mul:
                np.testing.assert_array_equal(y[sl], w * (w * x[sl]), err_msg=where)
        elif kind == "soc":
            e, l2 = 2.0 ** ((a - b) / 2), 2.0 ** ((a + b) / 2)
            r = dict(ref, eta=ref["eta"] * e, eta2=ref["eta2"] * e * e, lam=ref["lam"] * l2, lamterms=ref["lamterms"] * l2,
                     Hs=ref["Hs"] * e * e)
            kw = dict(lam=out["lam"][sl], w=out["w"][sl], eta=out["eta"][ci],
                      Hs=out["Hs"][hoff:hoff + (n * (n + 1) // 2 if n <= 4 else n)])
            if n > 4:
                e2 = -Kd[mp["soc_D"][2 * sidx]]
                assert Kd[mp["soc_D"][2 * sidx + 1]] == e2
                kw.update(u=Kd[mp["soc_u"][soff:soff + n]] / -e2, v=Kd[mp["soc_v"][soff:soff + n]] / -e2, eta2=e2)
            b_ = cr.soc_bounds(r)
            rat = cr.soc_ratios(r, **kw)
            if check_mul:
                J = np.r_[1.0, -np.ones(n - 1)]
                wr = r["w"]
                yref = r["eta2"] * (2 * wr * (wr @ x[sl]) - J * x[sl])
                yb = 2 * b_["eps"] * r["eta2"] * (2 * np.abs(wr) * (np.abs(wr) @ np.abs(x[sl])) + np.abs(x[sl]))
                rat["soc_mulHs"] = cr.ratio(y[sl] - yref, yb)
            _assert_within(WORST.add(rat, f"{where} SOC({n})"), f"{where} SOC({n})")
        else:
            k = c.dim
            R, Ri, lam = out["psd"][ipsd]
            ipsd += 1
            t = n
            # undo an exact scaling: R * 2^((b-a)/4), Rinv * 2^((a-b)/4), lam / 2^((a+b)/2), Hs / 2^(a-b)
            fr = 2.0 ** ((b - a) / 4)
            Hs = out["Hs"][hoff:hoff + t * (t + 1) // 2] / 2.0 ** (a - b)
            rat = cr.psd_ratios(ref, lam / 2.0 ** ((a + b) / 2), R * fr, Ri / fr, Hs)
            rat["K_Hs"] = cr.ratio(-Kd[mp["Hsblocks"][hoff:hoff + t * (t + 1) // 2]] / 2.0 ** (a - b) - cr.psd_hs(ref)[0],
                                   cr.psd_bounds(ref)["Hs"])
            if check_mul:
                yr, yb = cr.psd_mul_Hs(ref, x[sl])
                rat["mulHs"] = cr.ratio(y[sl] / 2.0 ** (a - b) - yr, yb)
                rat["mulHs_z"] = cr.ratio(yz[sl] - case.s[sl] * fs, cr.psd_mul_Hs(ref, case.z[sl])[1] * 2.0 ** a)
            _assert_within(WORST.add(rat, f"{where} PSD({k})"), f"{where} PSD({k})")


def _run(case, where, check_mul=True, factor_may_fail=False):
    """factor_may_fail: K of a late iterate (Hs condition ~1e24) may be refused by the factorisation; the scaling itself
    must be right either way"""
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(case.s, case.z) or factor_may_fail, where
    out = _read(ks)
    _check(case, ks, out, where, check_mul=check_mul)
    return ks, out


# ---- PSD sides -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", PSD_SIDES)
def test_psd_side_alone(k):
    _run(Case([("psd", k, "interior", 0)]), f"PSD({k}) alone")


def test_psd_every_side_in_one_handle():
    """LDS is sized by the largest side (psd_kmax) while each cone is laid out by its own k"""
    pieces = []
    for i, k in enumerate(PSD_SIDES):
        pieces += [("psd", k, "interior", 0), ("soc", (3, 65, 5)[i % 3], None, "both", i), ("nn", 1 + 37 * i % 11)]
    _run(Case(pieces, seed=3), "mixed sides")


@pytest.mark.parametrize("cls", [c for c in cr.PSD_CLASSES if c != "interior"])
@pytest.mark.parametrize("k", [47, 48])
def test_psd_spectrum_classes(k, cls):
    _run(Case([("nn", 5), ("psd", k, cls, 0), ("soc", 4, None, "both", 0)]), f"PSD({k}) {cls}", factor_may_fail=cls == "late")


# ---- second-order cones ------------------------------------------------------------------------------------------------
SOC_GROUPS = [
    (2, 3, 4, 5, 6),
    (63, 64, 65, 66),
    (127, 128, 129),
    (1000,),
    (4097,),
    (5, 64, 2, 129, 3, 65, 6, 128, 4),          # nine cones: three SOC workgroups, the last one part-filled
]


@pytest.mark.parametrize("delta", [None, 1e-2, 1e-6, 1e-10])
@pytest.mark.parametrize("dims", SOC_GROUPS, ids=["x".join(map(str, g)) for g in SOC_GROUPS])
def test_soc_dims_and_boundary_gaps(dims, delta):
    for which in (("both",) if delta is None else ("s", "z", "both")):
        pieces = []
        for i, n in enumerate(dims):
            pieces += [("nn", (255, 1, 256, 2)[i % 4]), ("soc", n, delta, which, i)]
        _run(Case(pieces, seed=len(dims)), f"SOC {dims} delta={delta} {which}")


# ---- elementwise cones at grid boundaries --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_nn_zero_grid_boundaries(m):
    pieces = [("zero", 3), ("nn", m - 3 - 4 - 3), ("soc", 4, None, "both", 1), ("nn", 3)]
    _run(Case(pieces), f"NN m={m}")
    pieces = [("nn", m // 2), ("soc", 65, None, "both", 2), ("zero", m - m // 2), ("psd", 2, "interior", 0),
              ("soc", 3, None, "both", 3)]
    _run(Case(pieces), f"NN m={m}+")


# ---- exact power-of-two scalings ---------------------------------------------------------------------------------------
SCALE_CASE = [("zero", 2), ("nn", 7), ("soc", 3, None, "both", 5), ("soc", 65, None, "both", 5), ("nn", 250),
              ("psd", 7, "interior", 0), ("soc", 129, 1e-6, "s", 5), ("psd", 48, "interior", 0), ("psd", 17, "cluster", 0)]


@pytest.mark.parametrize("a,b", [(4, -8), (128, -128), (-128, 128), (-64, -32), (100, 40)])
def test_scale_equivariance_is_exact(a, b):
    case = Case(SCALE_CASE, seed=11)
    k0 = _solver(case.cones)
    assert k0.kktsolver_update_from_sz(case.s, case.z)
    o0 = _read(k0)
    x = np.random.default_rng(5).standard_normal(len(case.s))
    y0 = k0.mul_Hs(x)
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(case.s * 2.0 ** a, case.z * 2.0 ** b)
    o = _read(ks)
    eq = lambda got, want, what: np.testing.assert_array_equal(got, want, err_msg=f"{what} at a={a} b={b}")
    soc = [i for i, c in enumerate(case.cones) if c.kind == 2]
    eq(o["eta"][soc], o0["eta"][soc] * 2.0 ** ((a - b) / 2), "eta")
    nn_rows = np.concatenate([np.arange(off, off + c.numel) for c, (off, *_r) in zip(case.cones, case.lay) if c.kind == 1])
    soc_rows = np.concatenate([np.arange(off, off + c.numel) for c, (off, *_r) in zip(case.cones, case.lay) if c.kind == 2])
    eq(o["w"][soc_rows], o0["w"][soc_rows], "SOC w")
    eq(o["w"][nn_rows], o0["w"][nn_rows] * 2.0 ** ((a - b) / 2), "NN w")
    eq(o["lam"], o0["lam"] * 2.0 ** ((a + b) / 2), "lambda")
    for (R, Ri, lam), (R0, Ri0, lam0) in zip(o["psd"], o0["psd"]):
        eq(R, R0 * 2.0 ** ((a - b) / 4), "R")
        eq(Ri, Ri0 * 2.0 ** ((b - a) / 4), "Rinv")
    eq(o["Hs"], o0["Hs"] * 2.0 ** (a - b), "Hs")
    mp = o["maps"]
    for key in ("Hsblocks", "soc_u", "soc_v", "soc_D"):
        eq(o["K"][mp[key]], o0["K"][mp[key]] * 2.0 ** (a - b), f"K[{key}]")
    eq(ks.mul_Hs(x), y0 * 2.0 ** (a - b), "mul_Hs")


@pytest.mark.parametrize("e", [300, -300])
def test_scale_extremes_are_right(e):
    """At s, z ~ 2^+-300 the products of squared column norms in the Jacobi sweep leave double range (at 2^300 they
    overflowed, every rotation was skipped and the update reported success with wrong singular values).  The update
    must succeed and match the reference, scaled exactly."""
    case = Case(SCALE_CASE, seed=11)
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(case.s * 2.0 ** e, case.z * 2.0 ** e)
    out = _read(ks)
    _check(case, ks, out, f"scale 2^{e}", scale=(e, e), check_mul=False)


# ---- level C: K from the caller's scaling ------------------------------------------------------------------------------
LEVEL_C = {
    "psd_sides": [p for i, k in enumerate(PSD_SIDES) for p in (("psd", k, "interior", 0), ("nn", 1 + i % 3))],
    "psd_classes": [("psd", k, c, 0) for k in (47, 48) for c in cr.PSD_CLASSES],
    "soc": [("nn", 255)] + [("soc", n, d, "both", 9) for n in (2, 3, 4, 5, 6, 63, 64, 65, 66, 127, 128, 129, 1000, 4097)
                            for d in (None, 1e-6)] + [("zero", 3)],
    "nn": [("zero", 100), ("nn", 413), ("soc", 3, None, "both", 4)],
}


@pytest.mark.parametrize("name", list(LEVEL_C))
def test_level_c_from_the_devices_own_scaling(name):
    from cuclarabel_amd.kktsolver import HipKKTSystem
    case = Case(LEVEL_C[name], seed=21)
    ka = _solver(case.cones)
    assert ka.kktsolver_update_from_sz(case.s, case.z) or name == "psd_classes"       # (late iterates: see _run)
    oa = _read(ka)
    R = np.concatenate([t[0].ravel(order="F") for t in oa["psd"]]) if oa["psd"] else np.zeros(0)
    Ri = np.concatenate([t[1].ravel(order="F") for t in oa["psd"]]) if oa["psd"] else np.zeros(0)
    kb = _solver(case.cones)
    sb = HipKKTSystem(kb)
    sb.init(np.zeros(2), np.zeros(len(case.s)))
    assert sb.update_scaling(oa["w"], oa["eta"], oa["lam"], R, Ri) or name == "psd_classes"
    Kb = kb.KKT().data
    mp = oa["maps"]
    psd_hs = np.zeros(len(mp["Hsblocks"]), bool)
    for c, (off, hoff, *_r) in zip(case.cones, case.lay):
        if c.kind == 3:
            psd_hs[hoff:hoff + c.numel * (c.numel + 1) // 2] = True
    exact = np.ones(len(Kb), bool)
    exact[mp["Hsblocks"][psd_hs]] = False
    np.testing.assert_array_equal(Kb[exact], oa["K"][exact])
    ob = dict(oa, K=Kb.copy(), Hs=kb.get_Hs())
    _check(case, kb, ob, f"level C {name}", check_mul=False)


# ---- limits ------------------------------------------------------------------------------------------------------------
def test_psd_side_49_is_refused_and_48_accepted():
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for cones in ([PSDTriangleConeT(49)], [PSDTriangleConeT(48), NonnegativeConeT(3), PSDTriangleConeT(49)]):
        ks = _solver(cones)
        m = ks.m
        s = np.concatenate([cr.svec(np.eye(c.dim)) if c.kind == 3 else np.ones(c.numel) for c in cones])
        with pytest.raises(_lib.HipKKTError, match="side > 48"):
            ks.kktsolver_update_from_sz(s, s)
        sys_ = HipKKTSystem(ks)
        sys_.init(np.zeros(2), np.zeros(m))
        tot = sum(c.dim ** 2 for c in cones if c.kind == 3)
        with pytest.raises(_lib.HipKKTError, match="side > 48"):
            sys_.update_scaling(np.ones(m), np.ones(len(cones)), np.ones(m), np.zeros(tot), np.zeros(tot))
    _run(Case([("psd", 48, "interior", 0), ("nn", 3), ("psd", 2, "interior", 0)]), "side 48 accepted")


def test_psd_side_49_solves_at_level_b():
    """level B: the caller supplies Hs (here the oracle's) for a PSD(49) cone; the solve matches the oracle's"""
    from tests.oracle_bindings import OracleKKT
    cones = [NonnegativeConeT(4), PSDTriangleConeT(49), SecondOrderConeT(6)]
    rng = np.random.default_rng(49)
    m = sum(c.numel for c in cones)
    A = sp.random(m, 30, density=0.05, random_state=rng, data_rvs=rng.standard_normal).tocsc()
    P = sp.identity(30, format="csc")
    s49, z49 = cr.psd_pair(rng, 49)
    s6, z6 = cr.soc_pair(rng, 6)
    s = np.r_[cr.nn_point(rng, 4), s49, s6]
    z = np.r_[cr.nn_point(rng, 4), z49, z6]
    from cuclarabel_amd.kktsolver import HipKKTSolver
    ks = HipKKTSolver(P, A, cones)
    o = OracleKKT(P, A, cones, perm=ks.perm())
    assert o.update_scaling(s, z) and o.kktsolver_update()
    u, v, e2, _ = o.soc_sparse()
    assert ks.kktsolver_update(o.get_Hs(), u, v, e2)
    rx, rz = rng.standard_normal(30), rng.standard_normal(m)
    ks.kktsolver_setrhs(rx, rz)
    x, zz = np.zeros(30), np.zeros(m)
    assert ks.kktsolver_solve(x, zz)
    o.kktsolver_setrhs(rx, rz)
    ok, xo, zo = o.kktsolver_solve()
    assert ok
    scale = max(np.abs(xo).max(), np.abs(zo).max())
    assert max(np.abs(x - xo).max(), np.abs(zz - zo).max()) <= 1e-9 * scale


def test_failures_are_reported_without_nan_elsewhere():
    """a SOC boundary point at dim 65, and a singular PSD(48): the update returns False; the other cones' outputs stay
    finite and right"""
    case = Case([("nn", 300), ("soc", 65, None, "both", 1), ("soc", 5, None, "both", 2), ("psd", 8, "interior", 0)], seed=5)
    s = case.s.copy()
    off = case.lay[1][0]
    s[off + 1:off + 65] = s[off + 1:off + 65] / np.linalg.norm(s[off + 1:off + 65]) * s[off] * 2.0   # outside
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(s, case.z) is False
    out = _read(ks)
    keep = np.ones(len(s), bool)
    keep[off:off + 65] = False
    assert np.all(np.isfinite(out["w"][keep])) and np.all(np.isfinite(out["lam"][keep]))
    np.testing.assert_array_equal(out["w"][:300], np.sqrt(case.s[:300] / case.z[:300]))

    case = Case([("nn", 300), ("soc", 65, None, "both", 1), ("psd", 48, "interior", 0)], seed=6)
    s = case.s.copy()
    off = case.lay[2][0]
    G = np.random.default_rng(1).standard_normal((48, 48))
    S = G @ G.T / 48 + np.eye(48)
    S[-1, :] = S[:, -1] = 0.0                                        # singular: the last Cholesky pivot is exactly 0
    s[off:off + 48 * 49 // 2] = cr.svec(S)
    ks = _solver(case.cones)
    assert ks.kktsolver_update_from_sz(s, case.z) is False
    out = _read(ks)
    assert np.all(np.isfinite(out["w"][:off])) and np.all(np.isfinite(out["lam"][:off]))
    np.testing.assert_array_equal(out["w"][:300], np.sqrt(case.s[:300] / case.z[:300]))
    sl = slice(case.lay[1][0], case.lay[1][0] + 65)
    ref = case.refs[1][1]
    _assert_within(cr.soc_ratios(ref, lam=out["lam"][sl], w=out["w"][sl]), "SOC next to a singular PSD")
