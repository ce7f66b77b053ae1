"""Generalized power cones on the device: assembly against the numpy restatement, argument checks, the fused scaling
kernel against the float64 restatement and the extended-precision closed forms, mul_Hs, solves at levels B and C, a
point outside the dual cone, bit-reproducibility.

Device scaling bound.  For every cone the restatement's own relative error against the 60-digit closed forms is
measured (the largest over grad, d, p, q, r, the Hs block and the K columns), and the device is held to
MARGIN(n) times that plus FLOOR.  MARGIN(n) = 64 (1 + log2 n) for a cone of n rows: 64 is the margin the
exponential and power cones are held to (tests/test_gpu_nonsymmetric_cones.py) -- pow and sqrt on the device are a
few ulp from the host's, and each difference enters through the cancellation zeta = phi - ||w||^2 like the
restatement's own roundings, whose random-signed sum is what the restatement's error measures while the device's may be
worst-signed.  The factor 1 + log2 n is the operation count of the reduction: the host's running product rounds a
partial once per row, the device's fixed-order reduction (strided per lane, a butterfly over the 64 lanes, the four
waves of a workgroup) sends every row's factor through up to ceil(n / 64) + 8 <= 1 + log2 n (n <= 64) or a comparable
number of further roundings in ANOTHER order, so the two results differ by a rounding per level even where both are
equally accurate.  FLOOR = 16 ulp covers a restatement that happens to round exactly.  The scaling has no branch: no
point is left out.  The measured worst device / bound ratio is printed; DESIGN.md section 4.3 records it.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import _lib, ipm, problems
from cuclarabel_amd.cones import (GenPowerConeT, SecondOrderConeT, ZeroConeT, NonnegativeConeT, cone_kinds_dims,
                                  cone_param_ptr_vals)
from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
from tests import genpow_reference as G

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
FLOOR = 16 * EPS
ERR_ARG = -1          # HIPKKT_ERR_ARG


def margin(n):
    return 64.0 * (1.0 + np.log2(n))


def _create2(P, A, kinds, dims, pptr, pvals, which="ex2"):
    P = sp.triu(sp.csc_matrix(P), format="csc"); A = sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    h = C.c_void_p()
    st = _lib.default_settings()
    i64, f64, ptr = _lib.i64, _lib.f64, _lib.ptr
    a = [i64(P.indptr), i64(P.indices), f64(P.data), i64(A.indptr), i64(A.indices), f64(A.data)]
    kinds, dims = np.asarray(kinds, np.int32), np.asarray(dims, np.int64)
    L = _lib.lib()
    head = (C.byref(h), A.shape[1], A.shape[0], *[ptr(v) for v in a], len(kinds), ptr(kinds), ptr(dims))
    if which == "ex2":
        pp, pv = i64(pptr), f64(pvals)
        rc = L.hipkkt_kkt_create_ex2(*head, ptr(pp), ptr(pv), C.byref(st), 0)
    elif which == "ex":
        pv = f64(np.zeros(len(kinds)))
        rc = L.hipkkt_kkt_create_ex(*head, ptr(pv), C.byref(st), 0)
    else:
        rc = L.hipkkt_kkt_create(*head, C.byref(st), 0)
    msg = L.hipkkt_last_error().decode()
    if rc == 0:
        L.hipkkt_kkt_destroy(h)
    return rc, msg


def test_assembly_equals_the_numpy_restatement_for_interleaved_expansions():
    P, A, s, z = G.mixed_problem(11, G.MIXED)
    ks = HipKKTSolver(P, A, G.MIXED)
    S = G.expanded_structure(P, A, G.MIXED)
    assert ks.info["p"] == S["p"] == 13 and ks.N == S["N"]
    K = ks.KKT()
    np.testing.assert_array_equal(K.indptr, S["indptr"])
    np.testing.assert_array_equal(K.indices, S["indices"])
    maps = ks.maps()
    for k in ("P", "A", "Hsblocks", "diag_full", "soc_u", "soc_v", "soc_D", "dsigns", "genpow_p", "genpow_q", "genpow_r",
              "genpow_D"):
        np.testing.assert_array_equal(maps[k], S["maps"][k], err_msg=k)


def test_argument_errors():
    P, A = sp.identity(3, format="csc"), sp.identity(3, format="csc")
    ok = ([6], [3], [0, 2], [0.5, 0.5])
    assert _create2(P, A, *ok)[0] == 0
    for which in ("plain", "ex"):
        rc, msg = _create2(P, A, *ok, which=which)
        assert rc == ERR_ARG and "hipkkt_kkt_create_ex2" in msg
    for vals in ([0.5, 0.6], [1.5, -0.5], [0.0, 1.0], [0.5, float("nan")], [float("inf"), 0.5]):
        assert _create2(P, A, [6], [3], [0, 2], vals)[0] == ERR_ARG, vals
    assert _create2(P, A, [6], [3], [0, 3], [0.25, 0.25, 0.5])[0] == ERR_ARG          # dim2 = 0
    assert _create2(P, A, [6], [3], [0, 0], [])[0] == ERR_ARG                         # dim1 = 0
    assert _create2(P, A, [6], [3], [0, 1], [1.0])[0] == 0                            # dim1 = 1, dim2 = 2
    # the caller-scaled entry points have no way to receive p, q, r
    spec = GenPowerConeT([0.5, 0.5], 1)
    ks = HipKKTSolver(P, A, [spec])
    m = 3
    with pytest.raises(_lib.HipKKTError, match="generalized power"):
        ks.kktsolver_update(np.ones(3))
    system = HipKKTSystem(ks)
    system.init(np.zeros(3), np.zeros(3))
    with pytest.raises(_lib.HipKKTError, match="generalized power"):
        system.update_cones(np.ones(3), None, None, None, np.ones(m), np.ones(1), np.ones(m))
    with pytest.raises(_lib.HipKKTError, match="generalized power"):
        system.update_scaling(np.ones(m), np.ones(1), np.ones(m))
    # ... and the handle is still good for the device-scaled route
    ks.set_nonsymmetric_scaling(ipm.DUAL, 1.0)
    zz = np.array([1.0, 1.2, 0.1])
    assert ks.kktsolver_update_from_sz(zz, zz)


def _scaling_cases():
    rng = np.random.default_rng(23)
    shapes = G.SHAPES + ((1, 63), (63, 1), (64, 1), (1, 64), (65, 2), (3, 65), (32, 32), (31, 32), (33, 32), (200, 312),
                         (256, 257), (300, 400), (10, 600))
    out = []
    for d1, d2 in shapes:
        spec = G.random_spec(rng, d1, d2)
        out.append((spec,) + G.random_interior_pair(spec, rng))
        out.append((spec,) + G.central_pair(spec, rng))
    return out


def test_device_scaling_against_restatement_and_extended_precision():
    cases = _scaling_cases()
    specs = [c[0] for c in cases]
    s = np.concatenate([c[1] for c in cases])
    z = np.concatenate([c[2] for c in cases])
    m = len(z)
    ks = HipKKTSolver(sp.identity(m, format="csc"), sp.identity(m, format="csc"), specs)
    mu = 0.37
    for strategy in (ipm.DUAL, ipm.PRIMAL_DUAL):            # mu is read under both
        ks.set_nonsymmetric_scaling(strategy, mu)
        assert ks.kktsolver_update_from_sz(s, z)
        dev = ks.genpow()
        Hs_d, Kv, maps = ks.get_Hs(), ks.KKT().data, ks.maps()
        cones = G.scale_cones(specs, s, z, mu)
        worst = (0.0, None)
        o = oq = orr = 0
        smu = np.sqrt(mu)
        for k, (c, spec) in enumerate(zip(cones, specs)):
            zc = z[c.rng]
            ref = G.mp_closed(spec, zc)                       # grad, d, p, q, r
            host = (c.grad, c.d, c.p, c.q, c.r)
            err_r = max(G.rel_err(h, r) for h, r in zip(host, ref))
            err_d = max(G.rel_err(d, r) for d, r in zip(dev[k], ref))
            # the Hs block and the K values: mu d, -sqrt(mu) (q, r, p), (-1, -1, +1)
            n, d1, d2 = c.n, c.d1, c.d2
            err_d = max(err_d, G.rel_err(Hs_d[c.rng] / mu, ref[1]),
                        G.rel_err(-Kv[maps["Hsblocks"][c.rng]] / mu, ref[1]),
                        G.rel_err(Kv[maps["genpow_p"][o:o + n]] / -smu, ref[2]),
                        G.rel_err(Kv[maps["genpow_q"][oq:oq + d1]] / -smu, ref[3]),
                        G.rel_err(Kv[maps["genpow_r"][orr:orr + d2]] / -smu, ref[4]) if np.any(zc[d1:]) else 0.0)
            np.testing.assert_array_equal(Kv[maps["genpow_D"][3 * k:3 * k + 3]], [-1.0, -1.0, 1.0])
            o, oq, orr = o + n, oq + d1, orr + d2
            bound = margin(n) * err_r + FLOOR
            if err_d / bound > worst[0]:
                worst = (err_d / bound, (spec.dim1, spec.dim2, err_d, err_r))
            assert err_d <= bound, (spec.dim1, spec.dim2, err_d, err_r)
        print("strategy", strategy, "worst device error / bound %.3g at (dim1, dim2, device, restatement)" % worst[0], worst[1])


def test_mul_Hs_against_the_dense_Hs_of_the_read_back():
    pb = problems.generalized_power_mix(copies=2)
    ks = HipKKTSolver(pb.P, pb.A, pb.cones)
    rng = np.random.default_rng(3)
    z = pb.z0.copy()
    for c in ipm._make_cones(pb.cones):                       # off the unit point: w != 0
        if isinstance(c, ipm._GenPow):
            w = rng.standard_normal(c.d2)
            z[c.off + c.d1:c.off + c.n] = 0.5 * w / np.linalg.norm(w)
    mu = 0.9
    ks.set_nonsymmetric_scaling(ipm.DUAL, mu)
    assert ks.kktsolver_update_from_sz(z, z)
    x = rng.standard_normal(pb.m)
    y = ks.mul_Hs(x)
    recs = iter(ks.genpow())
    for c in ipm._make_cones(pb.cones):
        if not isinstance(c, ipm._GenPow):
            np.testing.assert_array_equal(y[c.rng], 0.0)
            continue
        _, d, p, q, r = next(recs)
        H = np.diag(d) + np.outer(p, p)
        H[:c.d1, :c.d1] -= np.outer(q, q)
        H[c.d1:, c.d1:] -= np.outer(r, r)
        ref = mu * (H @ x[c.rng])
        # the three dot products and the dense product sum the same n terms in different orders: n eps of the
        # magnitudes summed
        mag = mu * (np.abs(d) * np.abs(x[c.rng]) + (np.abs(p) @ np.abs(x[c.rng])) * np.abs(p)
                    + np.concatenate([(np.abs(q) @ np.abs(x[c.rng][:c.d1])) * np.abs(q),
                                      (np.abs(r) @ np.abs(x[c.rng][c.d1:])) * np.abs(r)]))
        assert np.all(np.abs(y[c.rng] - ref) <= 2 * c.n * EPS * mag + 1e-300), (c.d1, c.d2)


def _reduced_solution(P, A, cones, rx, rz):
    Kr = G.reduced_matrix(P, A, cones)
    sol = np.linalg.solve(Kr, np.concatenate([rx, rz]))
    return sol, np.linalg.cond(Kr)


def test_level_b_solve_against_the_reduced_dense_system():
    P, A, s, z = G.mixed_problem(11, G.MIXED)
    mu = 0.7
    ks = HipKKTSolver(P, A, G.MIXED)
    ks.set_nonsymmetric_scaling(ipm.DUAL, mu)
    assert ks.kktsolver_update_from_sz(s, z)
    rng = np.random.default_rng(5)
    rx, rz = rng.standard_normal(ks.n), rng.standard_normal(ks.m)
    ks.kktsolver_setrhs(rx, rz)
    x, zz = np.zeros(ks.n), np.zeros(ks.m)
    assert ks.kktsolver_solve(x, zz)
    sol, cond = _reduced_solution(P, A, G.scale_cones(G.MIXED, s, z, mu), rx, rz)
    # refinement stops at a residual of 1e-12 + 1e-13 ||b|| (the settings' defaults): the error is at most cond times that
    tol = cond * (1e-12 + 1e-13 * np.abs(np.concatenate([rx, rz])).max()) * 10
    print("cond", cond, "err", np.abs(np.concatenate([x, zz]) - sol).max(), "tol", tol)
    assert np.abs(np.concatenate([x, zz]) - sol).max() <= tol
    assert ks.fallbacks == (0, 0)


# (the batched call is the affine step by definition)
@pytest.mark.parametrize("mode,affine", [("eager", True), ("eager", False), ("lazy", True), ("lazy", False),
                                         ("batched", True), ("torch", True), ("torch", False)])
def test_level_c_solve_in_every_mode_against_the_reduced_dense_system(mode, affine):
    """(The symmetric cones' step is held to its defining equations at rounding level in tests/test_gpu_system_step.py.)"""
    P, A, s, z = G.mixed_problem(13, G.MIXED)
    rng = np.random.default_rng(7)
    n, m = P.shape[0], A.shape[0]
    q, b = rng.standard_normal(n), rng.standard_normal(m)
    x = rng.standard_normal(n)
    tau, kappa, mu = 1.3, 0.7, 0.8
    rhs_x, rhs_z = rng.standard_normal(n), rng.standard_normal(m)
    rhs_s = s.copy() if affine else rng.standard_normal(m)
    rhs_tau, rhs_kappa = 0.4, -0.2
    ks = HipKKTSolver(P, A, G.MIXED)
    system = HipKKTSystem(ks)
    if mode == "torch":
        system.staging = "torch"
    system.init(q, b)
    ks.set_nonsymmetric_scaling(ipm.DUAL, mu)
    if mode == "lazy":
        assert system.update(s, z)
        system.set_lazy(True)
    if mode == "batched":
        ok, step = system.update_and_solve_affine(rhs_x, rhs_z, rhs_tau, rhs_kappa, x, s, z, tau, kappa)
    else:
        assert system.update(s, z)
        ok, step = system.solve(rhs_x, rhs_s, rhs_z, rhs_tau, rhs_kappa, x, s, z, tau, kappa, affine)
    assert ok and ks.fallbacks == (0, 0)
    dx, dz, ds, dtau, dkappa = step
    # kkt_solve! (kktsystem.jl:135-215) on the host with dense reduced solves
    cones = G.scale_cones(G.MIXED, s, z, mu)
    Kr = G.reduced_matrix(P, A, cones)
    cond = np.linalg.cond(Kr)
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pf = (Pt + sp.triu(Pt, 1).T).toarray()
    sol2 = np.linalg.solve(Kr, np.concatenate([-q, b]))
    x2, z2 = sol2[:n], sol2[n:]
    const = s.copy() if affine else np.concatenate([c.ds_from_dz_offset(rhs_s[c.rng], z[c.rng]) for c in cones])
    sol1 = np.linalg.solve(Kr, np.concatenate([rhs_x, const - rhs_z]))
    x1, z1 = sol1[:n], sol1[n:]
    xi = x / tau
    tnum = rhs_tau - rhs_kappa / tau + q @ x1 + b @ z1 + 2 * (xi @ (Pf @ x1))
    xm = xi - x2
    tden = kappa / tau - q @ x2 - b @ z2 + xm @ (Pf @ xm) - x2 @ (Pf @ x2)
    dtau_h = tnum / tden
    dx_h, dz_h = x1 + dtau_h * x2, z1 + dtau_h * z2
    ds_h = -(np.concatenate([c.mul_Hs(dz_h[c.rng]) for c in cones]) + const)
    dkappa_h = -(rhs_kappa + kappa * dtau_h) / tau
    # as at level B: cond times the refinement's stopping residual, through a handful of further operations
    scale = max(1.0, np.abs(sol1).max(), np.abs(sol2).max())
    tol = 100 * cond * 1e-12 * scale * max(1.0, abs(dtau_h))
    print(mode, affine, "cond %.3g tol %.3g" % (cond, tol), "errs", abs(dtau - dtau_h), np.abs(dx - dx_h).max(),
          np.abs(dz - dz_h).max(), np.abs(ds - ds_h).max())
    assert abs(dtau - dtau_h) <= tol and abs(dkappa - dkappa_h) <= tol
    for a_, b_ in ((dx, dx_h), (dz, dz_h), (ds, ds_h)):
        assert np.abs(a_ - b_).max() <= tol * max(1.0, np.abs(b_).max())


def test_a_point_outside_the_dual_cone_is_reported_and_the_handle_survives():
    specs = [GenPowerConeT([0.4, 0.6], 2), GenPowerConeT(problems.normalised_alphas(np.ones(300)), 400)]
    rng = np.random.default_rng(9)
    pairs = [G.random_interior_pair(c, rng) for c in specs]
    z = np.concatenate([p[1] for p in pairs])
    m = len(z)
    ks = HipKKTSolver(sp.identity(m, format="csc"), sp.identity(m, format="csc"), specs)
    ks.set_nonsymmetric_scaling(ipm.DUAL, 1.0)
    assert ks.kktsolver_update_from_sz(z, z)
    good = ks.KKT().data.copy()
    for bad_row, val in ((0, -0.1), (3, 50.0), (4 + 7, -1.0), (4 + 300 + 5, 1e6)):     # z_i <= 0 and zeta <= 0, both cones
        zb = z.copy()
        zb[bad_row] = val
        assert ks.kktsolver_update_from_sz(zb, zb) is False
    assert ks.kktsolver_update_from_sz(z, z)
    np.testing.assert_array_equal(ks.KKT().data, good)


def test_two_runs_give_bit_identical_K_values():
    pb = problems.generalized_power_mix(copies=2)
    out = []
    for _ in range(2):
        ks = HipKKTSolver(pb.P, pb.A, pb.cones)
        ks.set_nonsymmetric_scaling(ipm.DUAL, 0.6)
        assert ks.kktsolver_update_from_sz(pb.s0, pb.z0)
        assert ks.kktsolver_update_from_sz(pb.s0, pb.z0)
        out.append((ks.KKT().data.copy(), [np.concatenate(r) for r in ks.genpow()]))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        np.testing.assert_array_equal(a, b)


def test_level_a_with_a_caller_expanded_K():
    """Level A: the caller owns K and Dsigns.  The restatement's expanded K goes in as is (no zero cone, so that K is
    quasi-definite without a regulariser)."""
    from cuclarabel_amd.kktsolver import HipDirectLDLSolver
    specs = G.MIXED[:-1]
    P, A, s, z = G.mixed_problem(17, specs)
    cones = G.scale_cones(specs, s, z, 0.5)
    S = G.expanded_structure(P, A, specs)
    vals = G.expanded_values(S, cones)
    K = sp.csc_matrix((vals, S["indices"], S["indptr"]), shape=(S["N"], S["N"]))
    ldl = HipDirectLDLSolver(K, S["maps"]["dsigns"])
    assert ldl.refactor()
    rng = np.random.default_rng(1)
    b = np.concatenate([rng.standard_normal(S["n"] + S["m"]), np.zeros(S["p"])])
    x = np.zeros(S["N"])
    ldl.solve(K, x, b)
    Kf = G.expanded_matrix(S, vals).toarray()
    ref = np.linalg.solve(Kf, b)
    cond = np.linalg.cond(Kf)
    # one LDL' solve without refinement: N eps cond, with a factor 10
    print("level A err", np.abs(x - ref).max(), "cond", cond)
    assert np.abs(x - ref).max() <= 10 * S["N"] * EPS * cond * max(1.0, np.abs(ref).max())
    assert ldl.fallbacks == (0, 0)
