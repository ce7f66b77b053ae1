"""Exponential and power cones on the device: assembly, argument checks, the scaling kernel against the float64
restatement and the extended-precision oracle, mul_Hs, the entry-point rules, points outside the cone, equilibration.

Device scaling bound.  For every point the restatement's own relative error against mpmath is measured (the largest
of grad, H_dual and Hs), and the device is held to MARGIN times that plus FLOOR ulp.  MARGIN = 64: the device sums in
the same order (the kernel file is built without FMA contraction), so what differs is log / exp / pow / sqrt being a
few ulp from the host's; each such difference enters through the same cancellations as the restatement's own
roundings, of which a cone's scaling has a few dozen -- the restatement's error is their random-signed sum, 64 covers
their worst-signed one.  FLOOR = 16 ulp covers a restatement that happens to round exactly.
Measured worst ratios (device error / bound) on the MI355X are printed by the test; see DESIGN.md section 4.3.
"""
import ctypes as C

import numpy as np
import pytest

from cuclarabel_amd import _lib, ipm, problems
from cuclarabel_amd.cones import (ExponentialConeT, PowerConeT, SecondOrderConeT, ZeroConeT, NonnegativeConeT,
                                  cone_kinds_dims, cone_params)
from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
from tests import nonsymmetric_reference as R
from tests.golden import nonsymmetric_fixtures as F

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN, FLOOR = 64.0, 16 * EPS
ERR_ARG = -1          # HIPKKT_ERR_ARG


def _create(P, A, kinds, dims, params=None, ex=True):
    import scipy.sparse as sp
    P = sp.triu(sp.csc_matrix(P), format="csc"); A = sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    h = C.c_void_p()
    st = _lib.default_settings()
    i64, f64, ptr = _lib.i64, _lib.f64, _lib.ptr
    a = [i64(P.indptr), i64(P.indices), f64(P.data), i64(A.indptr), i64(A.indices), f64(A.data)]
    kinds, dims = np.asarray(kinds, np.int32), np.asarray(dims, np.int64)
    L = _lib.lib()
    if ex:
        par = None if params is None else f64(params)
        rc = L.hipkkt_kkt_create_ex(C.byref(h), A.shape[1], A.shape[0], *[ptr(v) for v in a], len(kinds), ptr(kinds),
                                    ptr(dims), ptr(par), C.byref(st), 0)
    else:
        rc = L.hipkkt_kkt_create(C.byref(h), A.shape[1], A.shape[0], *[ptr(v) for v in a], len(kinds), ptr(kinds),
                                 ptr(dims), C.byref(st), 0)
    msg = L.hipkkt_last_error().decode()
    if rc == 0:
        L.hipkkt_kkt_destroy(h)
    return rc, msg


def test_assembly_maps_equal_the_soc3_twin():
    pb = R.mixed_six()
    ks = HipKKTSolver(pb.P, pb.A, pb.cones)
    tw = HipKKTSolver(pb.P, pb.A, R.soc3_twin(pb.cones))
    assert ks.info["p"] == tw.info["p"] and ks.info["nHs"] == tw.info["nHs"] and ks.N == tw.N
    ma, mb = ks.maps(), tw.maps()
    for k in ma:
        np.testing.assert_array_equal(ma[k], mb[k], err_msg=k)
    Ka, Kb = ks.KKT(), tw.KKT()
    np.testing.assert_array_equal(Ka.indptr, Kb.indptr)
    np.testing.assert_array_equal(Ka.indices, Kb.indices)
    off = pb.n + sum(c.numel for c in pb.cones[:-5])
    np.testing.assert_array_equal(ma["dsigns"][off:off + 15], -1)


def test_argument_errors():
    import scipy.sparse as sp
    P, A = sp.identity(3, format="csc"), sp.identity(3, format="csc")
    rc, msg = _create(P, A, [5], [3], ex=False)
    assert rc == ERR_ARG and "hipkkt_kkt_create_ex" in msg
    assert _create(P, A, [4], [3], ex=False)[0] == 0                 # the plain constructor takes an exponential cone
    assert _create(P, A, [5], [3], [0.3])[0] == 0
    assert _create(P, A, [4], [3], None)[0] == 0                     # cone_params may be NULL without a power cone
    for alpha in (0.0, 1.0, -0.2, 1.5, float("nan")):
        assert _create(P, A, [5], [3], [alpha])[0] == ERR_ARG
    P4, A4 = sp.identity(4, format="csc"), sp.identity(4, format="csc")
    assert _create(P4, A4, [4], [4])[0] == ERR_ARG
    assert _create(P4, A4, [5], [4], [0.5])[0] == ERR_ARG
    assert _create(P, A, [6], [3])[0] == ERR_ARG


def _points():
    """[(spec, s, z, mu, strategy)]: every iterate of the two fixture runs (with the strategy the run used there) plus
    the random and central-path pairs, each under both strategies"""
    pts = R.fixture_points(F.basic_exp) + R.fixture_points(F.basic_pow)
    for kind in ("exp", "pow"):
        for spec, s, z in R.scaling_points(kind, 11, 40, 24):
            pts.append((spec, s, z, 0.0, ipm.PRIMAL_DUAL))
            pts.append((spec, s, z, 0.1 + (s @ z) / 3, ipm.DUAL))
    return pts


def test_device_scaling_against_restatement_and_extended_precision():
    pts = _points()
    # borderline guards are a condition: within a factor 10 of a threshold the device may take the other branch
    keep, sides = [], {}
    for p in pts:
        spec, s, z, mu, strategy = p
        c = ipm._make_cones([spec])[0]
        kind = "exp" if isinstance(spec, ExponentialConeT) else "pow"
        if strategy == ipm.PRIMAL_DUAL:
            gm = R.guard_margin(c.scaling_guards(s, z))
            if 0.1 <= gm <= 10.0:
                continue
            sides[(kind, gm > 10.0)] = sides.get((kind, gm > 10.0), 0) + 1
        keep.append(p)
    print("points", len(pts), "kept", len(keep), "sides", sides)
    assert len(pts) - len(keep) <= 0.05 * len(pts)
    for kind in ("exp", "pow"):
        assert sides.get((kind, True), 0) >= 20 and sides.get((kind, False), 0) >= 20, sides
    worst = {}
    for strategy in (ipm.PRIMAL_DUAL, ipm.DUAL):
        group = [p for p in keep if p[4] == strategy]
        # one handle per point keeps mu per point; a block-diagonal problem would share it.  Cheap: 3 rows each.
        for spec, s, z, mu, _ in group:
            import scipy.sparse as sp
            ks = HipKKTSolver(sp.identity(3, format="csc"), sp.identity(3, format="csc"), [spec])
            ks.set_nonsymmetric_scaling(strategy, mu)
            assert ks.kktsolver_update_from_sz(s, z), (spec, s, z)
            c = ipm._make_cones([spec])[0]
            assert c.update_scaling(s, z, mu, strategy)
            grad_d, H_d = ks.nonsymmetric()
            Hs_d = ks.get_Hs()
            st, H, Hs, used_pd, _ = R.mp_scaling(spec, s, z, mu, strategy)
            assert used_pd == c.used_primal_dual
            Hs_m = R.mp.matrix([Hs[0, 0], Hs[0, 1], Hs[1, 1], Hs[0, 2], Hs[1, 2], Hs[2, 2]])
            err_r = max(R.rel_err(c.grad, st), R.rel_err(c.H_dual, H), R.rel_err(c.get_Hs(), Hs_m))
            err_d = max(R.rel_err(grad_d[0], st), R.rel_err(H_d[0], H), R.rel_err(Hs_d, Hs_m))
            bound = MARGIN * err_r + FLOOR
            key = ("exp" if isinstance(spec, ExponentialConeT) else "pow", strategy)
            if err_d / bound > worst.get(key, (0,))[0]:
                worst[key] = (err_d / bound, err_d, err_r)
            assert err_d <= bound, (key, spec, s, z, err_d, err_r)
    for k, v in sorted(worst.items()):
        print("worst device error / bound", k, "ratio %.3g device %.3g restatement %.3g" % v)


def test_mul_Hs_and_many_cones_in_one_launch():
    """300 exponential and 300 power cones in one handle (several workgroups per list): Hs and mul_Hs per cone"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    specs = [ExponentialConeT() if j % 2 == 0 else PowerConeT(R.POW_ALPHAS[(j // 2) % 4]) for j in range(600)]
    pairs = [R.random_interior_pair(c, rng) for c in specs]
    s, z = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    m = 1800
    ks = HipKKTSolver(sp.identity(m, format="csc"), sp.identity(m, format="csc"), specs)
    assert ks.kktsolver_update_from_sz(s, z)
    cones = ipm._make_cones(specs)
    for c in cones:
        assert c.update_scaling(s[c.rng], z[c.rng], 0.0, ipm.PRIMAL_DUAL)
    Hs_h = np.concatenate([c.get_Hs() for c in cones])
    Hs_d = ks.get_Hs()
    np.testing.assert_allclose(Hs_d, Hs_h, rtol=1e-6, atol=0)          # g(s) stops at sqrt(eps): see the host test's header
    x = rng.standard_normal(m)
    y = ks.mul_Hs(x)
    y_h = np.concatenate([c.mul_Hs(x[c.rng]) for c in cones])
    # against the DEVICE's own blocks the product is three multiply-adds: a few ulp of the row's magnitude
    y_own = np.empty(m)
    for j, c in enumerate(cones):
        b = Hs_d[6 * j:6 * j + 6]
        M = np.array([[b[0], b[1], b[3]], [b[1], b[2], b[4]], [b[3], b[4], b[5]]])
        y_own[c.rng] = M @ x[c.rng]
        assert np.abs(y[c.rng] - y_own[c.rng]).max() <= 8 * EPS * np.abs(M).max() * np.abs(x[c.rng]).max()
    np.testing.assert_allclose(y, y_h, rtol=1e-6, atol=1e-6 * np.abs(y_h).max())
    # K carries -Hs in the cone's block
    K = ks.KKT().toarray()
    blk = -K[m:m + 3, m:m + 3]
    np.testing.assert_array_equal(np.triu(blk), np.triu(np.array([[Hs_d[0], Hs_d[1], Hs_d[3]], [0, Hs_d[2], Hs_d[4]], [0, 0, Hs_d[5]]])))


def test_scaling_entry_point_rules():
    pb = R.mixed_six()
    ks = HipKKTSolver(pb.P, pb.A, pb.cones)
    system = HipKKTSystem(ks)
    system.init(pb.q, pb.b)
    assert system.update(pb.s0, pb.z0)
    w, eta = ks.scaling_w()
    lam, psd = ks.scaling()
    with pytest.raises(_lib.HipKKTError, match="update_cones"):
        system.update_scaling(w, eta, lam, np.concatenate([p[0].ravel(order="F") for p in psd]),
                              np.concatenate([p[1].ravel(order="F") for p in psd]))
    with pytest.raises(_lib.HipKKTError):
        ks.set_nonsymmetric_scaling(2, 0.0)
    # on a symmetric handle the call is a no-op: K bit-identical
    sym = problems.small_mixed(seed=41)
    a, b = HipKKTSolver(sym.P, sym.A, sym.cones), HipKKTSolver(sym.P, sym.A, sym.cones)
    assert b.set_nonsymmetric_scaling(ipm.DUAL, 7.0)
    assert a.kktsolver_update_from_sz(sym.s0, sym.z0) and b.kktsolver_update_from_sz(sym.s0, sym.z0)
    np.testing.assert_array_equal(a.KKT().data, b.KKT().data)
    g, H = b.nonsymmetric()
    assert g.shape == (0, 3) and H.shape == (0, 3, 3)


@pytest.mark.parametrize("spec,zbad", [(ExponentialConeT(), [1.0, 1.0, 1.0]), (ExponentialConeT(), [-1.0, -5.0, 0.1]),
                                       (PowerConeT(0.6), [1.0, 1.0, 5.0]), (PowerConeT(0.6), [-1.0, 1.0, 0.1])], ids=str)
def test_point_outside_the_dual_cone_is_reported_and_the_handle_survives(spec, zbad):
    import scipy.sparse as sp
    rng = np.random.default_rng(3)
    s, z = R.random_interior_pair(spec, rng)
    ks = HipKKTSolver(sp.identity(3, format="csc"), sp.identity(3, format="csc"), [spec])
    c = ipm._make_cones([spec])[0]
    assert not c.is_dual_feasible(np.array(zbad))
    assert ks.kktsolver_update_from_sz(s, z)
    for strategy in (ipm.PRIMAL_DUAL, ipm.DUAL):
        ks.set_nonsymmetric_scaling(strategy, 0.5)
        assert ks.kktsolver_update_from_sz(s, np.array(zbad)) is False          # return value 1
        assert ks.kktsolver_update_from_sz(s, z)                                 # ... and a valid point still works
        rx, rz = rng.standard_normal(3), rng.standard_normal(3)
        ks.kktsolver_setrhs(rx, rz)
        x, zz = np.zeros(3), np.zeros(3)
        assert ks.kktsolver_solve(x, zz)
        K = ks.KKT()
        Kf = (K + sp.triu(K, 1).T).toarray()
        assert np.abs(Kf @ np.concatenate([x, zz]) - np.concatenate([rx, rz])).max() <= 1e-9 * max(1.0, np.abs(Kf).max())


def test_equilibrate_accepts_the_two_kinds():
    from cuclarabel_amd.equilibrate import equilibrate
    P, q, A, b, cones, _ = F.basic_exp()
    out = equilibrate(P, q, A, b, cones)
    P2, q2, A2, b2, cones2, _ = F.basic_pow()
    out2 = equilibrate(P2, q2, A2, b2, cones2)
    for o, cs in ((out, cones), (out2, cones2)):
        e = o[-1].e
        off = 0
        for c in cs:
            if isinstance(c, (ExponentialConeT, PowerConeT)):
                assert np.all(e[off:off + 3] == e[off]) and e[off] > 0       # one scalar per cone (coneops_defaults.jl:32-44)
            off += c.numel
