"""The seven _batch entry points of level C on stacks of independent member problems (tests/batch_reference.py): 1, 2, 3, 65
and 257 members, member boundaries inside, on and just past a wave, a workgroup of 256 and the 32 owner rows of the
residual pass, members with m = 0, with a zero cone only, second-order cones of 2 and 3 rows, PSD sides 1, 2 and 48, long
rows on both sides of a member boundary, and scalars that differ by decades between the members.

Exact, bit for bit: what is computed per row or per cone (add_step, combined_rhs, combined_ds, the five residual vectors)
equals the scalar twin called on the same handle with member b's scalars; the step length, an order-free minimum,
equals the scalar call on a handle that holds member b alone; a member with alpha = 0 keeps its rows; two calls agree.
Bounded, per member with the member's scalars and the bounds the scalar entry points are held to: the twelve residual
scalars (iterate_reference), the margins and the shifted vector (step_reference), the four defects of the affine and
the combined step (system_reference).  Simulated batch faults push those ratios above 1."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import batch_reference as B
from tests import iterate_reference as I
from tests import step_reference as sr
from tests import system_reference as S

pytestmark = pytest.mark.gpu

ALL_STACKS = tuple(B.SYSTEM_STACKS) + tuple(B.ITERATE_STACKS) + tuple(B.MANY)
CONE_STACKS = tuple(B.SYSTEM_STACKS) + tuple(B.MANY)
VEC = ("rx", "rz", "rx_inf", "rz_inf", "Px")


def _torch():
    import torch
    return torch


def up(a):
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.float64)
    t = torch.zeros(max(a.size, 1), dtype=torch.float64, device="cuda")
    t[:a.size] = torch.from_numpy(a)
    torch.cuda.synchronize()
    return t[:a.size]


def new(k):
    torch = _torch()
    t = torch.full((max(k, 1),), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t[:k]


def down(ks, t):
    ks.synchronize()
    return t.cpu().numpy().copy()


def p(t):
    return t.data_ptr()


def _sample(nb, k=10):
    """members to compare against handles of their own: all of a small stack, a spread of a large one"""
    return list(range(nb)) if nb <= k else sorted(set(np.linspace(0, nb - 1, k).astype(int).tolist() + [1, nb - 2]))


# ------------------------------------------------------------------------------------------------ residuals and the elementwise steps
@pytest.mark.parametrize("name", ALL_STACKS)
def test_residuals_vectors_equal_the_twin_and_the_scalars_are_the_members_own(name):
    st = B.stack(name)
    ks, system = st.handle()
    x, s, z, tau = B.residual_data(st)
    tx, ts, tz = up(x), up(s), up(z)

    def run():
        out = {k: new(st.n if k in ("rx", "rx_inf", "Px") else st.m) for k in VEC}
        scal = system.residuals_batch_dev(p(tx), p(ts), p(tz), tau, *(p(out[k]) for k in VEC))
        return {k: down(ks, v) for k, v in out.items()}, scal
    vec, scal = run()
    vec2, scal2 = run()
    assert scal.tobytes() == scal2.tobytes() and all(vec[k].tobytes() == vec2[k].tobytes() for k in VEC), "two calls differ"
    assert scal.shape == (st.nb, 12)
    worst = {}
    for b in range(st.nb):
        twin = {k: new(st.n if k in ("rx", "rx_inf", "Px") else st.m) for k in VEC}
        system.residuals_dev(p(tx), p(ts), p(tz), float(tau[b]), *(p(twin[k]) for k in VEC))
        cut = B.cut_vectors(st, b, vec)
        for k, v in B.cut_vectors(st, b, {k: down(ks, t) for k, t in twin.items()}).items():
            assert cut[k].tobytes() == v.tobytes(), f"{name} member {b}: {k} differs from the scalar call with tau[b]"
        if st.nb <= 3 or b in _sample(st.nb, 24):
            for k, v in B.residual_ratios(st, b, x, s, z, tau, cut, scal[b]).items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= 1.0, f"{name} member {b}: {k} error / bound = {v}"
    print(f"{name}: largest error / bound per scalar", {k: f"{v:.3g}" for k, v in sorted(worst.items())})
    assert ks.fallbacks == (0, 0)


@pytest.mark.parametrize("name", ALL_STACKS)
def test_combined_rhs_and_add_step_equal_the_twin_and_alpha_zero_leaves_the_rows(name):
    st = B.stack(name)
    ks, system = st.handle()
    rng = np.random.default_rng(5)
    rx, rz = rng.standard_normal(st.n), rng.standard_normal(st.m)
    sigma = 1.0 - B.spread(st.nb, -8, 0, 6)
    trx, trz = up(rx), up(rz)
    ox, oz = new(st.n), new(st.m)
    assert system.combined_rhs_batch_dev(p(ox), p(oz), p(trx), p(trz), sigma)
    gx, gz = down(ks, ox), down(ks, oz)
    x, s, z = rng.standard_normal(st.n), rng.standard_normal(st.m), rng.standard_normal(st.m)
    x[::7] = -0.0                                         # (v + 0 d would turn these into +0.0)
    dx, ds, dz = rng.standard_normal(st.n), rng.standard_normal(st.m), rng.standard_normal(st.m)
    alpha = np.array([(0.0, 1e-3, 1.0)[(b + b // 3) % 3] for b in range(st.nb)])
    tdx, tds, tdz = up(dx), up(ds), up(dz)

    def step():
        tx, ts, tz = up(x), up(s), up(z)
        assert system.add_step_batch_dev(p(tx), p(ts), p(tz), p(tdx), p(tds), p(tdz), alpha)
        return down(ks, tx), down(ks, ts), down(ks, tz)
    ax, as_, az = step()
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip((ax, as_, az), step())), "two calls differ"
    for b in range(st.nb):
        xr, zr = st.xr(b), st.zr(b)
        tx2, tz2 = new(st.n), new(st.m)
        assert system.combined_rhs_dev(p(tx2), p(tz2), p(trx), p(trz), float(sigma[b]))
        assert gx[xr].tobytes() == down(ks, tx2)[xr].tobytes() and gz[zr].tobytes() == down(ks, tz2)[zr].tobytes(), (name, b)
        if alpha[b] == 0.0:
            assert ax[xr].tobytes() == x[xr].tobytes() and as_[zr].tobytes() == s[zr].tobytes() and az[zr].tobytes() == z[zr].tobytes()
        else:
            tx, ts, tz = up(x), up(s), up(z)
            assert system.add_step_dev(p(tx), p(ts), p(tz), p(tdx), p(tds), p(tdz), float(alpha[b]))
            assert ax[xr].tobytes() == down(ks, tx)[xr].tobytes() and as_[zr].tobytes() == down(ks, ts)[zr].tobytes() and \
                az[zr].tobytes() == down(ks, tz)[zr].tobytes(), (name, b)
    assert ks.fallbacks == (0, 0)


# ------------------------------------------------------------------------------------------------ the cone operations
@pytest.mark.parametrize("name", CONE_STACKS)
def test_combined_ds_and_step_length_per_member(name):
    st = B.stack(name)
    its = B.interior(st)
    s, z = st.cat_z([it.s for it in its]), st.cat_z([it.z for it in its])
    ks, system = st.handle(update=(s, z))
    dz, ds = B.seeded_steps(st, its)
    tdz, tds, tz, ts = up(dz), up(ds), up(z), up(s)
    sigma_mu, m_corr = B.spread(st.nb, -7, 1, 11), B.spread(st.nb, -3, 0, 12)
    out = new(st.m)
    assert system.combined_ds_batch_dev(p(out), p(tdz), p(tds), sigma_mu, m_corr)
    got = down(ks, out)
    out2 = new(st.m)
    assert system.combined_ds_batch_dev(p(out2), p(tdz), p(tds), sigma_mu, m_corr)
    assert got.tobytes() == down(ks, out2).tobytes(), "two calls differ"
    for b in range(st.nb):
        twin = new(st.m)
        assert system.combined_ds_dev(p(twin), p(tdz), p(tds), float(sigma_mu[b]), float(m_corr[b]))
        assert got[st.zr(b)].tobytes() == down(ks, twin)[st.zr(b)].tobytes(), f"{name} member {b}: combined_ds differs from the twin"
    # step length: the members' own tau, kappa and steps of both signs
    rng = np.random.default_rng(13)
    tau, kappa = np.array([it.tau for it in its]), np.array([it.kappa for it in its])
    dtau, dkappa = tau * rng.uniform(-3, 1, st.nb), kappa * rng.uniform(-3, 1, st.nb)
    alpha = system.step_length_batch_dev(p(tdz), p(tds), p(tz), p(ts), dtau, dkappa, tau, kappa)
    assert alpha.tobytes() == system.step_length_batch_dev(p(tdz), p(tds), p(tz), p(ts), dtau, dkappa, tau, kappa).tobytes()
    assert alpha.shape == (st.nb,)
    for b in _sample(st.nb):
        pb, it = st.members[b], its[b]
        ks1, sys1 = B.alone(pb, update=(it.s, it.z))
        t1 = [up(v) for v in (dz[st.zr(b)], ds[st.zr(b)], it.z, it.s)]          # (kept alive over the call)
        a1 = sys1.step_length_dev(p(t1[0]), p(t1[1]), p(t1[2]), p(t1[3]), float(dtau[b]), float(dkappa[b]), float(tau[b]),
                                  float(kappa[b]))
        assert alpha[b] == a1, f"{name} member {b}: step length {alpha[b]!r} != {a1!r} of the member alone"
    if st.nb == 1:
        assert alpha[0] == system.step_length_dev(p(tdz), p(tds), p(tz), p(ts), float(dtau[0]), float(dkappa[0]), float(tau[0]),
                                                  float(kappa[0]))
    assert ks.fallbacks == (0, 0)


@pytest.mark.parametrize("primal", (True, False))
@pytest.mark.parametrize("name", CONE_STACKS)
def test_shift_to_interior_per_member(name, primal):
    """member b's branch is chosen by ITS margins and degree: members outside their cones, with small margins and well
    inside sit side by side"""
    st = B.stack(name)
    its = B.interior(st)
    ks, system = st.handle()
    parts = []
    for b, (pb, it) in enumerate(zip(st.members, its)):
        base = it.s if primal else it.z
        mode = b % 3
        parts.append(base - 2.0 * np.abs(base).max(initial=1.0) if mode == 0 else 1e-2 * base if mode == 1 else 1e3 * base)
    v = st.cat_z(parts)

    def run():
        t = up(v)
        mg = system.shift_to_interior_batch_dev(p(t), primal)
        return mg, down(ks, t)
    mg, got = run()
    mg2, got2 = run()
    assert mg.tobytes() == mg2.tobytes() and got.tobytes() == got2.tobytes(), "two calls differ"
    assert mg.shape == (st.nb, 2)
    seen = set()
    for b in (range(st.nb) if st.nb <= 3 else _sample(st.nb, 30)):
        pb, zr = st.members[b], st.zr(b)
        ref = sr.shift_ref(pb.cones, v[zr], primal)
        assert ref["branch"] is not None, (name, b)
        seen.add(ref["branch"])
        ratios = {"min": ref["min"].ratio(mg[b, 0]), "pos": I.ratio(abs(mg[b, 1] - ref["pos"]), ref["bpos"]),
                  "shift": I.ratio(np.abs(got[zr] - ref["value"]), ref["bound"])}
        assert max(ratios.values()) <= 1.0, f"{name} member {b} ({ref['branch']}): {ratios}"
        zero = sr.unit_rows(pb.cones)[1]
        assert np.all(got[zr][zero] == 0.0) if primal else got[zr][zero].tobytes() == v[zr][zero].tobytes()
    assert st.nb < 3 or {"outside", "good"} <= seen
    if st.nb == 1:
        t = up(v)
        assert system.shift_to_interior_dev(p(t), primal)[0] == mg[0, 0]
    assert ks.fallbacks == (0, 0)


# ------------------------------------------------------------------------------------------------ the solves
def _solve_both(st, system, ks, its, rhss):
    x = st.cat_x([it.x for it in its])
    s, z = st.cat_z([it.s for it in its]), st.cat_z([it.z for it in its])
    rx, rs, rz = st.cat_x([r.x for r in rhss]), st.cat_z([r.s for r in rhss]), st.cat_z([r.z for r in rhss])
    tau, kappa = np.array([it.tau for it in its]), np.array([it.kappa for it in its])
    rt, rk = np.array([r.tau for r in rhss]), np.array([r.kappa for r in rhss])
    tx, ts, tz, trx, trs, trz = (up(v) for v in (x, s, z, rx, rs, rz))
    steps = []
    for affine in (True, False):
        dx, ds, dz = new(st.n), new(st.m), new(st.m)
        ok, dtau, dkappa = system.solve_batch_dev((p(dx), p(ds), p(dz)), (p(trx), p(ts if affine else trs), p(trz)), rt, rk,
                                                  (p(tx), p(ts), p(tz)), tau, kappa, affine)
        assert ok
        steps.append((down(ks, dx), down(ks, dz), down(ks, ds), dtau, dkappa))
    return steps


@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("name", tuple(B.SYSTEM_STACKS) + ("many65",))
def test_solve_batch_meets_the_four_defects_per_member(name, lazy):
    st = B.stack(name)
    its = B.interior(st)
    rhss = B.rhs_of(st, its)
    ks, system = st.handle()
    if lazy:
        system.set_lazy(True)                           # the constant-RHS solve is pending when the affine solve_batch arrives
    assert system.update(st.cat_z([it.s for it in its]), st.cat_z([it.z for it in its]))
    steps = _solve_both(st, system, ks, its, rhss)
    again = _solve_both(st, system, ks, its, rhss)
    for a, b_ in zip(steps, again):
        assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b_)), "two calls differ"
    worst = {}
    for b in (range(st.nb) if st.nb <= 3 else _sample(st.nb, 8)):
        view = B.member_view(st, b, ks)
        for affine, (dx, dz, ds, dtau, dkappa) in zip((True, False), steps):
            step = (dx[st.xr(b)], dz[st.zr(b)], ds[st.zr(b)], float(dtau[b]), float(dkappa[b]))
            r = S.step_ratios(view, its[b], rhss[b], step, affine)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(r.values()) <= 1.0, (name, b, "affine" if affine else "combined", r)
    print(f"{name} lazy={lazy}: largest defect / bound", {k: f"{v:.3g}" for k, v in sorted(worst.items())})
    assert ks.fallbacks == (0, 0)


# ------------------------------------------------------------------------------------------------ the bounds bite
@pytest.mark.parametrize("fault", ("neighbour_rows", "joint_tau"))
def test_a_simulated_batch_fault_exceeds_the_bounds(fault):
    """the restatement without a fault sits within the bounds; with member b's scalars taken over member b + 1's rows, or the
    joint tau used for every member, a ratio exceeds 1 -- for the residual scalars / vectors and for the step's defects"""
    st = B.stack("three")
    x, s, z, tau = B.residual_data(st)
    for b in range(st.nb):
        vec, scal = B.restate_member(st, b, x, s, z, tau)
        assert max(B.residual_ratios(st, b, x, s, z, tau, vec, scal).values()) <= 1.0
        vec, scal = B.restate_member(st, b, x, s, z, tau, fault=fault)
        assert max(B.residual_ratios(st, b, x, s, z, tau, vec, scal).values()) > 1.0, (fault, b)
    its = B.interior(st)
    rhss = B.rhs_of(st, its)
    ks, system = st.handle(update=(st.cat_z([it.s for it in its]), st.cat_z([it.z for it in its])))
    views = {b: B.member_view(st, b, ks) for b in range(st.nb)}
    for b in (0, 2):
        for affine in (True, False):
            good = B.faulty_step(st, b, views, its, rhss, affine, None)
            assert max(S.step_ratios(views[b], its[b], rhss[b], good, affine).values()) <= 1.0
            bad = B.faulty_step(st, b, views, its, rhss, affine, fault)
            assert max(S.step_ratios(views[b], its[b], rhss[b], bad, affine).values()) > 1.0, (fault, b, affine)


# ------------------------------------------------------------------------------------------------ refusals
def _batch_calls(system, st, t):
    one = np.ones(max(system.nb, st.nb))
    return {
        "residuals": lambda a=one: system.residuals_batch_dev(p(t["x"]), p(t["s"]), p(t["z"]), a, p(t["rx"]), p(t["rz"]), p(t["rxi"]),
                                                              p(t["rzi"]), p(t["Px"])),
        "solve": lambda a=one: system.solve_batch_dev((p(t["dx"]), p(t["ds"]), p(t["dz"])), (p(t["rx"]), p(t["s"]), p(t["rz"])), a, one,
                                                      (p(t["x"]), p(t["s"]), p(t["z"])), one, one, True),
        "combined_ds": lambda a=one: system.combined_ds_batch_dev(p(t["ds"]), p(t["dz"]), p(t["rz"]), a, one),
        "step_length": lambda a=one: system.step_length_batch_dev(p(t["dz"]), p(t["ds"]), p(t["z"]), p(t["s"]), a, one, one, one),
        "shift": lambda a=one: system.shift_to_interior_batch_dev(p(t["rzi"]), True),
        "combined_rhs": lambda a=one: system.combined_rhs_batch_dev(p(t["dx"]), p(t["dz"]), p(t["rx"]), p(t["rz"]), a),
        "add_step": lambda a=one: system.add_step_batch_dev(p(t["x"]), p(t["s"]), p(t["z"]), p(t["dx"]), p(t["ds"]), p(t["dz"]), a),
    }


def test_refusals_leave_the_handle_usable():
    from cuclarabel_amd import _lib
    from cuclarabel_amd.cones import ExponentialConeT, NonnegativeConeT, PSDTriangleConeT
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    st = B.stack("three")
    its = B.interior(st)
    s, z = st.cat_z([it.s for it in its]), st.cat_z([it.z for it in its])
    ks = HipKKTSolver(st.P, st.A, st.cones)
    system = HipKKTSystem(ks)
    system.staging = "torch"
    system.init(st.q, st.b)
    assert system.update(s, z)
    rng = np.random.default_rng(3)
    t = {k: up(rng.standard_normal(st.n)) for k in ("x", "dx", "rx", "rxi", "Px")}
    t.update({k: up(rng.standard_normal(st.m)) for k in ("dz", "ds", "rz", "rzi")})
    t["s"], t["z"] = up(s), up(z)
    before = {k: down(ks, v) for k, v in t.items()}
    # every _batch call before set_problems
    for name, call in _batch_calls(system, st, t).items():
        with pytest.raises(_lib.HipKKTError, match="partition"):
            call()
    # coupling entries: the first member's last column handed to the second member (its P and A entries now couple the two)
    (n0, m0), (n1, m1) = st.blocks[0], st.blocks[1]
    with pytest.raises(_lib.HipKKTError, match="couples member 0 with member 1"):
        system.set_problems([(n0 - 1, m0), (n1 + 1, m1)] + st.blocks[2:])
    with pytest.raises(_lib.HipKKTError, match="x_off ends"):
        system.set_problems(st.blocks[:-1])
    for name, call in _batch_calls(system, st, t).items():           # still no partition
        with pytest.raises(_lib.HipKKTError, match="partition"):
            call()
    assert all(down(ks, v).tobytes() == before[k].tobytes() for k, v in t.items()), "a refused call wrote something"
    assert ks.fallbacks == (0, 0)
    # a NULL scalar array
    system.set_problems(st.blocks)
    for name, call in _batch_calls(system, st, t).items():
        if name == "shift":
            continue
        with pytest.raises(_lib.HipKKTError):
            call(None)
    assert all(down(ks, v).tobytes() == before[k].tobytes() for k, v in t.items()), "a refused call wrote something"
    assert ks.fallbacks == (0, 0)
    # ... and a following valid call succeeds
    alpha = system.step_length_batch_dev(p(t["dz"]), p(t["ds"]), p(t["z"]), p(t["s"]), np.ones(st.nb), np.ones(st.nb), np.ones(st.nb),
                                         np.ones(st.nb))
    assert alpha.shape == (st.nb,) and np.all((alpha > 0) & (alpha <= 1))
    system.set_problems(None)                                        # cleared
    with pytest.raises(_lib.HipKKTError, match="partition"):
        system.add_step_batch_dev(p(t["x"]), p(t["s"]), p(t["z"]), p(t["dx"]), p(t["ds"]), p(t["dz"]), np.ones(st.nb))
    # handles outside the batched set
    for cones, large in (([NonnegativeConeT(2), ExponentialConeT()], False), ([PSDTriangleConeT(49)], True)):
        m = sum(c.numel for c in cones)
        k2 = HipKKTSolver(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((m, 2))), cones, large_psd=large)
        s2 = HipKKTSystem(k2)
        s2.init(np.zeros(2), np.zeros(m))
        with pytest.raises(_lib.HipKKTError, match="exponential" if not large else "side 48"):
            s2.set_problems([(2, m)])
        assert k2.fallbacks == (0, 0)
    assert ks.fallbacks == (0, 0)
