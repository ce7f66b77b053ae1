"""Problems with exponential and power cones through the device backends: level C against the host algebra on a
problem with all six cone kinds, the lazy and the batched route against the plain one, the reference's two known
answers through every backend, and entropy maximisation with 20 000 cones against the CPU path."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import ipm, problems
from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
from tests import nonsymmetric_reference as R
from tests.golden import nonsymmetric_fixtures as F
from tests.oracle_bindings import OracleKKT

pytestmark = pytest.mark.gpu


def _host_cones(pb, s, z, mu, strategy):
    cones = ipm._make_cones(pb.cones)
    for c in cones:
        args = (mu, strategy) if isinstance(c, ipm._NonSym) else ()
        assert c.update_scaling(s[c.rng].copy(), z[c.rng].copy(), *args)
    return cones


@pytest.mark.parametrize("strategy", [ipm.PRIMAL_DUAL, ipm.DUAL])
@pytest.mark.parametrize("affine", [True, False])
def test_device_kkt_solve_matches_host_algebra_with_all_six_kinds(affine, strategy):
    """As tests/test_ipm_fixtures.py::test_device_kkt_solve_matches_host_algebra, same 1e-9 bound, on a problem that
    also holds exponential and power cones; and hipkkt_kkt_mul_Hs against the host cones."""
    pb = R.mixed_six()
    ks = HipKKTSolver(pb.P, pb.A, pb.cones)
    system = HipKKTSystem(ks)
    system.init(pb.q, pb.b)
    rng = np.random.default_rng(17)
    s, z = pb.s0, pb.z0
    x = rng.standard_normal(pb.n)
    tau, kappa, mu = 1.3, 0.7, 0.9
    ks.set_nonsymmetric_scaling(strategy, mu)
    assert system.update(s, z)
    rhs_x, rhs_z = rng.standard_normal(pb.n), rng.standard_normal(pb.m)
    rhs_s = s.copy() if affine else rng.standard_normal(pb.m)
    rhs_tau, rhs_kappa = 0.4, -0.2
    ok, (dx, dz, ds, dtau, dkappa) = system.solve(rhs_x, rhs_s, rhs_z, rhs_tau, rhs_kappa, x, s, z, tau, kappa, affine)
    assert ok
    # ---- the same on the host: the oracle's K^{-1} on the SOC(3) twin, values from the host cone objects
    cones = _host_cones(pb, s, z, mu, strategy)
    ipm.adopt_device_scaling(cones, ks.scaling()[1])          # a PSD cone's scaled space: see the test this one follows
    o = OracleKKT(pb.P, pb.A, R.soc3_twin(pb.cones), perm=ks.perm())
    assert o.kktsolver_update_values(*ipm.host_cone_data(cones)[:4])
    v = rng.standard_normal(pb.m)
    y_h = np.concatenate([c.mul_Hs(v[c.rng]) for c in cones])
    np.testing.assert_allclose(ks.mul_Hs(v), y_h, rtol=0, atol=1e-9 * max(1.0, np.abs(y_h).max()))

    def each(fn, *vecs):
        out = np.empty(pb.m)
        for c in cones:
            out[c.rng] = fn(c, *[w[c.rng] for w in vecs])
        return out

    def ksolve(rx, rz):
        o.kktsolver_setrhs(rx, rz)
        ok_, xo, zo = o.kktsolver_solve()
        assert ok_
        return xo, zo

    Pt = sp.triu(sp.csc_matrix(pb.P), format="csc")
    Pfull = (Pt + sp.triu(Pt, 1).T).tocsr()
    x2, z2 = ksolve(-pb.q, pb.b)
    const = s.copy() if affine else each(lambda c, d, zz: c.ds_from_dz_offset(d, zz), rhs_s, z)
    x1, z1 = ksolve(rhs_x, const - rhs_z)
    xi = x / tau
    tnum = rhs_tau - rhs_kappa / tau + pb.q @ x1 + pb.b @ z1 + 2 * (xi @ (Pfull @ x1))
    xm = xi - x2
    tden = kappa / tau - pb.q @ x2 - pb.b @ z2 + xm @ (Pfull @ xm) - x2 @ (Pfull @ x2)
    dtau_h = tnum / tden
    dx_h, dz_h = x1 + dtau_h * x2, z1 + dtau_h * z2
    ds_h = -(each(lambda c, w: c.mul_Hs(w), dz_h) + const)
    dkappa_h = -(rhs_kappa + kappa * dtau_h) / tau
    assert abs(dtau - dtau_h) <= 1e-9 * max(1.0, abs(dtau_h))
    assert abs(dkappa - dkappa_h) <= 1e-9 * max(1.0, abs(dkappa_h))
    for a, b in ((dx, dx_h), (dz, dz_h), (ds, ds_h)):
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())


def test_lazy_batched_and_host_cone_routes_agree_with_the_plain_one():
    pb = R.mixed_six(seed=43)
    rng = np.random.default_rng(19)
    x = rng.standard_normal(pb.n)
    rhs_x, rhs_z = rng.standard_normal(pb.n), rng.standard_normal(pb.m)
    mu = 0.8
    for strategy in (ipm.PRIMAL_DUAL, ipm.DUAL):
        out = []
        for route in ("plain", "batched", "lazy", "host_cones"):
            ks = HipKKTSolver(pb.P, pb.A, pb.cones)
            system = HipKKTSystem(ks)
            system.init(pb.q, pb.b)
            ks.set_nonsymmetric_scaling(strategy, mu)
            if route == "lazy":
                assert system.update(pb.s0, pb.z0)          # a first, eager update: lazy mode needs (x2, z2) once
                system.set_lazy(True)
            if route == "batched":
                ok, step = system.update_and_solve_affine(rhs_x, rhs_z, 0.4, -0.2, x, pb.s0, pb.z0, 1.3, 0.7)
            else:
                if route == "host_cones":
                    cones = _host_cones(pb, pb.s0, pb.z0, mu, strategy)
                    ref = HipKKTSolver(pb.P, pb.A, pb.cones)       # the PSD cones' scaled space from a device scaling
                    ref.set_nonsymmetric_scaling(strategy, mu)
                    assert ref.kktsolver_update_from_sz(pb.s0, pb.z0)
                    ipm.adopt_device_scaling(cones, ref.scaling()[1])
                    assert system.update_cones(*ipm.host_cone_data(cones))
                else:
                    assert system.update(pb.s0, pb.z0)
                ok, step = system.solve(rhs_x, pb.s0, rhs_z, 0.4, -0.2, x, pb.s0, pb.z0, 1.3, 0.7, True)
            assert ok, route
            assert ks.fallbacks == (0, 0)
            out.append(step)
        for route, other in zip(("batched", "lazy"), out[1:3]):
            for a, b in zip(out[0], other):
                np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * max(1.0, float(np.max(np.abs(a)))), err_msg=route)
        for a, b in zip(out[0], out[3]):      # host cone objects: the blocks agree to g(s)'s accuracy, not to round-off
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * max(1.0, float(np.max(np.abs(a)))))


def _check(r, exp):
    assert r.status == exp["status"] == ipm.SOLVED
    if exp["x"] is not None:
        assert np.linalg.norm(r.x - exp["x"]) <= F.ATOL
    assert abs(r.obj_val - exp["obj"]) <= F.ATOL


@pytest.mark.parametrize("backend", ["level_b", "level_c", "level_c_lazy", "level_c_host_cones", "level_c_batched"])
@pytest.mark.parametrize("fixture", [F.basic_exp, F.basic_pow], ids=lambda f: f.__name__)
def test_reference_known_answers_on_the_device(fixture, backend):
    P, q, A, b, cones, exp = fixture()
    be = {"level_b": lambda: ipm.HipBackend(P, A, cones),
          "level_c": lambda: ipm.HipSystemBackend(P, A, cones),
          "level_c_lazy": lambda: ipm.HipSystemBackend(P, A, cones, lazy=True),
          "level_c_host_cones": lambda: ipm.HipSystemBackend(P, A, cones, host_cones=True),
          "level_c_batched": lambda: ipm.HipSystemBackend(P, A, cones, batch_affine=True)}[backend]()
    r = ipm.solve(P, q, A, b, cones, be)
    print(backend, r.status, r.iterations, r.obj_val)
    _check(r, exp)
    assert be.ks.fallbacks == (0, 0)


def test_entropy_maximisation_with_20000_cones_device_against_cpu():
    pb = problems.entropy_maximization(20_000)
    be = ipm.HipSystemBackend(pb.P, pb.A, pb.cones)
    r_dev = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, be)
    r_cpu = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, R.OracleNonsymBackend(pb.P, pb.A, pb.cones))
    print("device", r_dev.status, r_dev.iterations, r_dev.obj_val, "cpu", r_cpu.status, r_cpu.iterations, r_cpu.obj_val)
    assert r_dev.status == ipm.SOLVED and r_cpu.status == ipm.SOLVED
    # both stop at the 1e-8 gap tolerance; the feasibility residuals enter the objective too: 100 x that
    assert abs(r_dev.obj_val - r_cpu.obj_val) <= 1e-6 * max(1.0, abs(r_cpu.obj_val))
    assert be.ks.fallbacks == (0, 0)
