"""The static regulariser and the failure words per member (hipkkt_kkt_system_set_member_status; csrc/batch_kernels.hip:
k_member_diag_max, k_member_eps, k_member_pivot_scan; the three regulariser sites of csrc/factor_kernels.hip; the cone
scaling's failure sites in csrc/kernels.hip) through level B on a partitioned handle, so that (s, z) and the right-hand
side are free.  The stacks and the model are those of tests/member_status_reference.py; tests/
test_member_status_reference_host.py checks the model on the CPU and shows that its seeded faults are caught.

Settings: static regularisation 1e-8 + 1e-3 max |K_ii| (a large proportional part: the members' eps_b lie orders of
magnitude apart), dynamic regularisation at its default 1e-13 -- every pivot of these stacks is far above it.

  eps       eps_b == what a handle that holds member b ALONE reports after an update with the same rows of (s, z), and within
            1 ulp of numpy's c0 + c1 * max (two roundings).  Members of 1, 255, 256, 257 image rows; nb = 1, 3, 5, 300;
            maxima at a first row, a last row, a negative -Hs entry, an expansion row, the stack's in another member.
  pivots    refinement off: member b's rows of hipkkt_kkt_solve equal the dense (K_b + eps_b S_b)^-1 rhs_b within
            100 cond(K_b + eps_b S_b) 2^-52 of the solution's size; the same solve with the mode off lies >= 1e6 tolerances
            away (the host test shows that on the CPU for the joint epsilon).
  nb = 1    update, eps, hipkkt_kkt_solve and hipkkt_kkt_system_solve are == with the mode on and off.
  words     a second-order cone with z0 < ||z1||, a nonnegative row with z < 0 (NaN in Hs), a PSD block that is not positive
            definite, in the first, a middle and the last member of 3 and of 300: the word of that member alone, the
            update returns failure, the others' rows of a following solve under member refinement are what they are when
            the member is healthy, and an interior update clears every word.  Non-finite values are data here.
"""
import numpy as np
import pytest

from tests import member_refinement_cases as mc
from tests import member_status_reference as ms
from tests import residual_reference as rr

pytestmark = pytest.mark.gpu

_H = {}


def solver(P, A, cones, refine):
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver
    return HipKKTSolver(P, A, cones, settings=_lib.default_settings(**ms.settings(refine)))


def handle(st, refine=False):
    """(ks, system, rows) for a stack: partitioned, both member modes off; once per session"""
    key = (st.name, refine)
    if key not in _H:
        from cuclarabel_amd.kktsolver import HipKKTSystem
        ks = solver(st.P, st.A, st.cones, refine)
        system = HipKKTSystem(ks)
        system.init(np.ones(st.n), np.ones(st.m))
        system.set_problems(st.blocks)
        rows, N = ms.member_rows(st)
        assert N == ks.N
        _H[key] = (ks, system, rows)
    return _H[key]


def level_b_solve(ks, st, b):
    ks.kktsolver_setrhs(b[:st.n], b[st.n:st.n + st.m])
    x, z = np.zeros(st.n), np.zeros(st.m)
    ok = ks.kktsolver_solve(x, z)
    return ok, np.concatenate([x, z])


def sample(nb):
    return range(nb) if nb <= 8 else sorted({0, 1, 2, 3, 10, 63, 64, 127, 128, 255, 256, 257, nb // 2, nb - 2, nb - 1})


# ------------------------------------------------------------------------------------------------ eps
@pytest.mark.parametrize("make", ms.EPS_CASES, ids=lambda f: f.__name__)
def test_every_members_epsilon_is_the_one_it_has_alone(make):
    st = make()
    ks, system, rows = handle(st)
    system.set_member_status(True)
    try:
        assert ks.kktsolver_update_from_sz(st.s, st.z)
        W = system.member_status()
    finally:
        system.set_member_status(False)
    assert W.shape == (st.nb, 3) and not W[:, :2].any()
    want = ms.member_eps(rr.sym_of(ks).diagonal(), rows)
    ulps = np.abs(W[:, 2] - want) / np.spacing(want)
    print(f"\n[member status] {st.name}: eps_b from {W[:, 2].min():.3e} to {W[:, 2].max():.3e}; against numpy at most "
          f"{ulps.max():.0f} ulp; {int((ulps == 0).sum())} of {st.nb} equal")
    assert ulps.max() <= 1.0
    assert ks.diagonal_regularizer == W[:, 2].max(), "hipkkt_kkt_last_regularizer reports the largest eps_b"
    for b in sample(st.nb):
        P, A, cones, s, z = ms.member_problem(st, b)
        alone = solver(P, A, cones, False)
        assert alone.kktsolver_update_from_sz(s, z)
        assert alone.diagonal_regularizer == W[b, 2], (st.name, b, alone.diagonal_regularizer, W[b, 2])
    # the mode off again: one epsilon, the stack's
    assert ks.kktsolver_update_from_sz(st.s, st.z)
    assert ks.diagonal_regularizer == W[:, 2].max()


def test_without_static_regularisation_nothing_is_added_and_eps_is_zero():
    from cuclarabel_amd import _lib
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    st = ms.case_three()
    ks = HipKKTSolver(st.P, st.A, st.cones, settings=_lib.default_settings(**dict(ms.settings(), static_regularization_enable=0)))
    system = HipKKTSystem(ks)
    system.init(np.ones(st.n), np.ones(st.m))
    system.set_problems(st.blocks)
    rows, N = ms.member_rows(st)
    b = mc.rhs(st, N, rows)
    assert ks.kktsolver_update_from_sz(st.s, st.z)
    ok0, x0 = level_b_solve(ks, st, b)
    system.set_member_status(True)
    assert ks.kktsolver_update_from_sz(st.s, st.z)
    W = system.member_status()
    ok1, x1 = level_b_solve(ks, st, b)
    assert ok0 and ok1 and not W.any() and ks.diagonal_regularizer == 0.0
    assert np.array_equal(x0, x1)


# ------------------------------------------------------------------------------------------------ pivots
def test_every_members_pivots_receive_its_own_epsilon():
    st = ms.case_three()
    ks, system, rows = handle(st)
    b = mc.rhs(st, ks.N, rows)
    system.set_member_status(True)
    try:
        assert ks.kktsolver_update_from_sz(st.s, st.z)
        W = system.member_status()
        ok, xz = level_b_solve(ks, st, b)
    finally:
        system.set_member_status(False)
    assert ok
    K, dsigns = rr.sym_of(ks), np.asarray(ks.maps()["dsigns"], np.float64)
    want, cond = ms.member_solve(K, dsigns, rows, W[:, 2], b)
    assert cond.max() < 1e3
    n_m = st.n + st.m

    def distance(x):
        return np.array([np.abs(x[r[r < n_m]] - want[r[r < n_m]]).max() / (ms.solve_tolerance(cond[k]) * np.abs(want[r]).max())
                         for k, r in enumerate(rows)])

    on = distance(xz)
    assert ks.kktsolver_update_from_sz(st.s, st.z)                 # the mode off: the joint epsilon on every pivot
    ok, xz_joint = level_b_solve(ks, st, b)
    off = distance(xz_joint)
    print(f"\n[member status] regularised solve, in tolerances of 100 cond 2^-52 (cond {cond}): mode on {on}, mode off {off}")
    assert on.max() <= 1.0, on
    others = [k for k in range(st.nb) if W[k, 2] != W[:, 2].max()]
    assert len(others) == 2 and all(off[k] >= 1e6 for k in others), off


# ------------------------------------------------------------------------------------------------ nb = 1
def test_one_member_is_bit_for_bit_the_handle_without_the_mode():
    import torch
    st = ms.case_one()
    ks, system, rows = handle(st, refine=True)
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    rng = np.random.default_rng(5)
    b = mc.rhs(st, ks.N, rows)
    sd, zd = up(st.s), up(st.z)
    var_x, rhs = up(rng.standard_normal(st.n)), [up(rng.standard_normal(k)) for k in (st.n, st.m, st.m)]
    p = lambda t: t.data_ptr()

    def run():
        assert ks.kktsolver_update_from_sz(st.s, st.z)
        out = dict(eps=ks.diagonal_regularizer, K=ks.KKT().data.copy())
        ok, out["xz"] = level_b_solve(ks, st, b)
        assert ok
        assert system.update_dev(p(sd), p(zd))
        lhs = [torch.zeros(max(k, 1), dtype=torch.float64, device=dev)[:k] for k in (st.n, st.m, st.m)]
        ok, dtau, dkappa = system.solve_dev(tuple(p(t) for t in lhs), tuple(p(t) for t in rhs), 0.3, 0.7,
                                            (p(var_x), p(sd), p(zd)), 1.1, 0.9, False)
        assert ok
        torch.cuda.synchronize()
        out["step"] = np.concatenate([t.cpu().numpy() for t in lhs] + [[dtau, dkappa]])
        out["ir"] = ks.last_ir_iterations
        return out

    off = run()
    system.set_member_status(True)
    try:
        on = run()
        W = system.member_status()
    finally:
        system.set_member_status(False)
    assert W.shape == (1, 3) and W[0, 2] == off["eps"] == on["eps"] and not W[0, :2].any()
    for key in ("K", "xz", "step"):
        assert np.array_equal(off[key], on[key]), key
    assert off["ir"] == on["ir"]


# ------------------------------------------------------------------------------------------------ the words
_ATTR = {}


def batch_step(system, T, st):
    """one affine kkt_solve! of the stack through hipkkt_kkt_system_solve_batch -> (ok, (dx, ds, dz) on the host)"""
    import torch
    p = lambda t: t.data_ptr()
    ok, dtau, dkappa = system.solve_batch_dev((p(T["dx"]), p(T["ds"]), p(T["dz"])), (p(T["rx"]), p(T["rz"]), p(T["rz"])),
                                              T["rtau"], T["rkappa"], (p(T["x"]), p(T["s"]), p(T["z"])), T["tau"], T["kappa"], True)
    torch.cuda.synchronize()
    return ok, np.concatenate([T["dx"].cpu().numpy(), T["ds"].cpu().numpy(), T["dz"].cpu().numpy()])


def attribution(nb):
    """the stack, its handle under both member modes, the healthy step and the members' tolerances: once per session"""
    if nb not in _ATTR:
        import torch
        st, where = ms.attribution_stack(nb)
        ks, system, rows = handle(st, refine=True)
        ks.set_stream(torch.cuda.current_stream().cuda_stream)       # (the tensors below are torch's)
        system.set_member_status(True)
        system.set_member_refinement(True)
        rng = np.random.default_rng(77 + nb)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
        T = dict(x=up(rng.standard_normal(st.n)), s=up(st.s), z=up(st.z), rx=up(rng.standard_normal(st.n)),
                 rz=up(rng.standard_normal(st.m)), dx=up(np.zeros(st.n)), ds=up(np.zeros(st.m)), dz=up(np.zeros(st.m)),
                 rtau=rng.uniform(0.5, 1.0, nb), rkappa=rng.uniform(0.5, 1.0, nb), tau=np.ones(nb), kappa=np.ones(nb))
        assert system.update_dev(T["s"].data_ptr(), T["z"].data_ptr())
        W = system.member_status()
        assert not W[:, :2].any()
        ok, step = batch_step(system, T, st)
        assert ok
        _, cond = ms.member_solve(rr.sym_of(ks), np.asarray(ks.maps()["dsigns"], np.float64), rows, W[:, 2], np.zeros(ks.N))
        _ATTR[nb] = (st, where, ks, system, rows, T, step, cond)
    return _ATTR[nb]


@pytest.mark.parametrize("kind", ("soc", "nn", "psd"))
@pytest.mark.parametrize("nb", (3, 300))
def test_a_failure_is_attributed_to_its_member_alone(nb, kind):
    import torch
    st, where, ks, system, rows, T, step0, cond = attribution(nb)
    x_off = np.concatenate([[0], np.cumsum([bl[0] for bl in st.blocks])])
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    for k in (0, nb // 2, nb - 1):
        s, z, poison = ms.poisoned(st, where, kind, k)
        sd, zd = up(s), up(z)
        ok = system.update_dev(sd.data_ptr(), zd.data_ptr())
        W = system.member_status()
        assert not ok, "the return value is the joint one: HIPKKT_NUMERIC_FAILURE"
        assert np.array_equal(W[:, :2], ms.member_words(st, poison)), (kind, k, np.argwhere(W[:, :2]))
        assert W[:, :2].any() == (not ok), "the OR over the members is the joint word"
        # the others' rows of a step behind the failed update, under member refinement: with both member modes on, a solve
        # that fails for member k still delivers every other member's rows
        ok2, step = batch_step(system, T, st)
        info = system.member_refinement_info()
        assert ok2 == (not info[:, 3].any()) and not np.delete(info[:, 3], k).any()
        if kind == "nn":
            assert not ok2 and info[k, 3] == 1.0, "the NaN block marks its member bad, and the solve's status is joint"
        worst = 0.0
        for j in range(nb):
            if j == k:
                continue
            own = np.concatenate([np.arange(x_off[j], x_off[j + 1]), st.n + np.arange(z_off[j], z_off[j + 1]),
                                  st.n + st.m + np.arange(z_off[j], z_off[j + 1])])
            worst = max(worst, np.abs(step[own] - step0[own]).max() / (ms.solve_tolerance(cond[j]) * np.abs(step0[own]).max()))
        print(f"\n[member status] nb {nb} {kind} in member {k}: the others' rows differ by {worst:.2e} tolerances")
        assert worst <= 1.0
        # an interior update clears every word
        assert system.update_dev(T["s"].data_ptr(), T["z"].data_ptr())
        assert not system.member_status()[:, :2].any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from cuclarabel_amd._lib import HipKKTError
    from cuclarabel_amd.kktsolver import HipKKTSystem
    st = ms.case_three()
    ks = solver(st.P, st.A, st.cones, False)
    system = HipKKTSystem(ks)
    system.init(np.ones(st.n), np.ones(st.m))
    with pytest.raises(HipKKTError, match="no partition"):
        system.set_member_status(True)
    system.set_problems(st.blocks)
    system.set_member_status(True)
    with pytest.raises(HipKKTError, match="no update"):
        system.member_status()
    assert ks.kktsolver_update_from_sz(st.s, st.z)
    assert system.member_status().shape == (3, 3)
    system.set_problems(st.blocks)                                 # a new partition clears the mode
    with pytest.raises(HipKKTError, match="not enabled"):
        system.member_status()
    system.set_member_status(True)
    system.set_member_status(False)
    with pytest.raises(HipKKTError, match="not enabled"):
        system.member_status()
    system.set_member_status(True)
    system.set_problems(None)                                      # ... and so does clearing it
    with pytest.raises(HipKKTError, match="not enabled"):
        system.member_status()
