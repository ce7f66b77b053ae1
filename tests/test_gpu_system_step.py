"""The level-C Newton step on the device against its four defining equations (tests/system_reference.py): reduced rows,
tau row, kappa and s row, each evaluated exactly from what the handle returned and held to an order-free bound, on
problems whose sizes sit on the lane and grid edges of the kernels between the solves (k_P_spmv*, k_dots*, k_sys_*,
k_neg_*, the addend path of k_mul_Hs*), through every route a step can take: eager update + solves (cached x2-only terms),
the lazy pair (seven dot pairs, (x2, z2) copied out of the 2-column solve), update_and_solve_affine, the host entry points,
second updates on the same handle and a change of P and A in between.

Out of scope on purpose: the elementwise kernels' grid cap of 4096 workgroups (a second lap above 2^20 rows)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import system_reference as S

pytestmark = pytest.mark.gpu

ROUTES = ("eager", "lazy", "batched", "host", "host_reuse")
_WORST = {}


def _handle(pb, lazy=False, staging="torch"):
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    ks = HipKKTSolver(pb.P, pb.A, pb.cones)
    system = HipKKTSystem(ks)
    system.staging = staging
    system.init(pb.q, pb.b)
    if lazy:
        system.set_lazy(True)
    return ks, system


def _iteration(pb, ks, system, it, rhs, route):
    """kkt_update!, kkt_solve!(:affine), kkt_solve!(:combined) of one iteration -> (affine step, combined step)"""
    var = (it.x, it.s, it.z, it.tau, it.kappa)
    if route == "batched":
        ok, aff = system.update_and_solve_affine(rhs.x, rhs.z, rhs.tau, rhs.kappa, *var)
    else:
        assert system.update(it.s, it.z)
        ok, aff = system.solve(rhs.x, it.s, rhs.z, rhs.tau, rhs.kappa, *var, True)
    assert ok
    ok, comb = system.solve(rhs.x, rhs.s, rhs.z, rhs.tau, rhs.kappa, *var, False, reuse_variables=(route == "host_reuse"))
    assert ok and ks.fallbacks == (0, 0)
    return aff, comb


def _check(tag, pb, ks, it, rhs, steps, Pfull=None):
    """all four defects of the affine and the combined step against the K and the scaling the handle holds now"""
    view = S.device_view(pb, ks)
    for affine, (dx, dz, ds, dtau, dkappa) in zip((True, False), steps):
        r = S.step_ratios(view, it, rhs, (dx, dz, ds, dtau, dkappa), affine, Pfull=Pfull)
        print(f"{tag} {'affine' if affine else 'combined'}: defect / bound", {k: f"{v:.3g}" for k, v in sorted(r.items())})
        for k, v in r.items():
            _WORST[(tag.split()[0], k)] = max(_WORST.get((tag.split()[0], k), 0.0), v)
        assert max(r.values()) <= 1.0, (tag, affine, r)
    assert ks.fallbacks == (0, 0)


def _route_handle(pb, route):
    return _handle(pb, lazy=(route == "lazy"), staging=("host" if route.startswith("host") else "torch"))


@pytest.mark.parametrize("scale", S.SCALES)
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_on_the_mixed_problem(route, scale):
    pb = S.problem("mixed")
    it, = (S.iterate(pb, scale),)
    rhs = S.rhs_for(pb, it)
    ks, system = _route_handle(pb, route)
    steps = _iteration(pb, ks, system, it, rhs, route)
    _check(f"{route} mixed/{scale}", pb, ks, it, rhs, steps)


@pytest.mark.parametrize("scale", S.SCALES)
def test_affine_step_of_the_lazy_pair_is_the_eager_one_bit_for_bit(scale):
    """a column of a 2-column solve ends where its single solve ends; the seven-pair step kernel adds in the order of the
    cached terms"""
    pb = S.problem("mixed")
    it = S.iterate(pb, scale)
    rhs = S.rhs_for(pb, it)
    out = []
    for route in ("eager", "lazy"):
        ks, system = _route_handle(pb, route)
        out.append(_iteration(pb, ks, system, it, rhs, route))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("route", ("eager", "lazy"))
def test_second_update_and_new_P_and_A_on_the_same_handle(route):
    """a stale cached term, a stale (x2, z2) or a stale P behind vmap shows in defects (1) and (2) of the later steps"""
    pb = S.problem("mixed")
    ks, system = _route_handle(pb, route)
    it1, it2 = S.iterate(pb, "unit"), S.iterate(pb, "late", S.ITERATE_SEED + 10)
    for tag, it in (("first", it1), ("second", it2)):
        rhs = S.rhs_for(pb, it)
        _check(f"{route} {tag}-update", pb, ks, it, rhs, _iteration(pb, ks, system, it, rhs, route))
    # new values of P and A, then a third iteration: the spmv must read the new P
    P2, A2 = pb.P.copy(), pb.A.copy()
    P2.data = P2.data * 1.25
    A2.data = A2.data * np.where(np.arange(A2.nnz) % 2 == 0, 0.75, 1.5)
    ks.kktsolver_update_P(P2)
    ks.kktsolver_update_A(A2)
    pb2 = S.Problem("mixed2", P2, A2, pb.cones, 7101 + 1)
    assert np.array_equal(pb2.q, pb.q) and np.array_equal(pb2.b, pb.b)
    it3 = S.iterate(pb, "unit", S.ITERATE_SEED + 20)
    rhs = S.rhs_for(pb, it3)
    _check(f"{route} new-P-A", pb2, ks, it3, rhs, _iteration(pb2, ks, system, it3, rhs, route))


@pytest.mark.parametrize("route", ("eager", "lazy"))
@pytest.mark.parametrize("name", S.EDGE_BUILDERS)
def test_edge_builders(name, route):
    pb = S.problem(name)
    ks, system = _route_handle(pb, route)
    for scale in S.SCALES:                              # (the late iterate doubles as a second update on the same handle)
        it = S.iterate(pb, scale)
        rhs = S.rhs_for(pb, it)
        _check(f"{route} {name}/{scale}", pb, ks, it, rhs, _iteration(pb, ks, system, it, rhs, route))


@pytest.mark.parametrize("route", ("eager", "lazy"))
def test_large_builder_second_laps(route):
    """n = 2048 * 32 + 33 and m = 64 * 256 + 257: the second lap of the spmv grid and of k_dots.  (Every column of A needs
    an entry, so its rows hold three to five, not one or two.)"""
    pb = S.problem("large")
    ks, system = _route_handle(pb, route)
    it = S.iterate(pb, "unit")
    rhs = S.rhs_for(pb, it)
    _check(f"{route} large/unit", pb, ks, it, rhs, _iteration(pb, ks, system, it, rhs, route))


@pytest.mark.parametrize("staging", ("torch", "host"))
@pytest.mark.parametrize("name", ("lp1", "lp33", "lp257", "n1", "n33", "n257", "large"))
def test_initial_point_equals_the_level_b_solves_bit_for_bit(name, staging):
    """QP branch: (-q, b) -> (x, z), s = -z.  LP branch (P empty): (0, b) -> (x, -s), then (-q, 0) -> z.  The right-hand
    sides are data, so nothing is rounded before the solves: no tolerance."""
    pb = S.problem(name)
    ks, system = _handle(pb, staging=staging)
    it = S.iterate(pb, "unit")
    assert system.update(it.s, it.z)
    ok, x, s, z = system.solve_initial_point()
    assert ok and np.isfinite(x).all() and np.isfinite(s).all() and np.isfinite(z).all()

    def solve(rx, rz):
        ks.kktsolver_setrhs(rx, rz)
        xo, zo = np.zeros(pb.n), np.zeros(pb.m)
        assert ks.kktsolver_solve(xo, zo)
        return xo, zo
    assert S.initial_point_mismatches(pb, solve, x, s, z) == 0
    assert ks.fallbacks == (0, 0)


def test_zz_report_the_largest_ratio_per_route_and_defect():
    for (route, k), v in sorted(_WORST.items()):
        print(f"largest defect / bound  route {route:10s} defect ({k}): {v:.3g}")
    assert all(v <= 1.0 for v in _WORST.values())
