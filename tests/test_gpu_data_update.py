"""The data updates of level C on the device (hipkkt_kkt_system_set_equilibration, hipkkt_kkt_system_update_data_P / _A /
_q / _b, hipkkt_kkt_system_data_norms) against tests/data_update_reference.py, with == after every step: K's values
through hipkkt_kkt_get_values, the image the residual reads probed as tests/test_gpu_kkt_values.py probes it, q and b
through hipkkt_kkt_system_residuals at x = s = z = 0, tau = 1 (rx = -q, rz = -b), -q through the constant-RHS solves.

The sequences are the model's own (data_update_reference.SEQUENCES; tests/test_data_update_reference_host.py shows that
each seeded fault of the model is caught by them): written through a current image, not into a dirty one, one and two
kpos slots, indexed-all equals vector, stale state refused.  Edges here: k and vector lengths 1, 255, 256, 257, one
length past the kernels' grid cap, scalings over eight decades with c != 1, scalings cleared, a partitioned handle, every
refusal."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import data_update_reference as du
from tests import kvalue_reference as kv

pytestmark = pytest.mark.gpu


class Device:
    """a handle with its level-C system under the model's method names"""

    def __init__(self, case, q=None, b=None, init=True):
        import torch
        from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
        self.torch = torch
        self.case = case
        self.ks = HipKKTSolver(case.P, case.A, case.cones)
        self.system = HipKKTSystem(self.ks)
        self.dev = self.system._devstr
        self.n, self.m = self.ks.n, self.ks.m
        if init:
            self.system.init(q, b)
        new = lambda k: torch.zeros(max(k, 1), dtype=torch.float64, device=self.dev)
        self.zx, self.zs, self.zz = new(self.n), new(self.m), new(self.m)
        self.out = [new(self.n) for _ in range(3)] + [new(self.m) for _ in range(2)]      # rx, rx_inf, Px | rz, rz_inf

    @property
    def handle(self):
        return self.ks

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)
        self.torch.cuda.synchronize()
        return t

    def _refusable(self, fn, *args):
        from cuclarabel_amd._lib import HipKKTError
        try:
            return fn(*args)
        except HipKKTError as err:
            assert "(-1)" in str(err), err                       # HIPKKT_ERR_ARG, nothing else
            m = re.search(r"index\[(\d+)\]", str(err))
            raise du.Refused(str(err), int(m.group(1)) if m else None) from None

    def set_equilibration(self, d=None, e=None, c=1.0):
        from cuclarabel_amd.equilibrate import Equilibration
        self.system.set_equilibration(None if d is None and e is None else Equilibration(d, None, e, None, c))

    def update_data(self, which, values, index=None):
        v = np.asarray(values, np.float64).ravel()
        t = self.up(v)
        fn = getattr(self.system, f"update_data_{which}_dev")
        self._refusable(fn, t.data_ptr() if v.size else 0, index, v.size)

    def level_b_update_P(self, vals):
        self.ks.kktsolver_update_P(vals)

    def system_update(self, Hs, u=(), v=(), eta2=()):
        """hipkkt_kkt_system_update_cones with the case's Hs blocks; the NT scaling beside them is not part of the value path"""
        cones = self.case.cones
        eye = np.concatenate([np.eye(c.dim).ravel() for c in cones if c.kind == 3] + [np.zeros(0)])
        ok = self.system.update_cones(Hs, u, v, eta2, np.ones(self.m), np.ones(len(cones)), np.ones(self.m), eye, eye)
        if not ok:
            raise kv.ValuePathError("update", "the level-C update reported a numeric failure")
        return ok

    def solve(self):
        rng = np.random.default_rng(91)
        p = lambda t: t.data_ptr()
        lhs = [self.up(np.zeros(max(k, 1))) for k in (self.n, self.m, self.m)]
        rhs = [self.up(rng.standard_normal(max(k, 1))) for k in (self.n, self.m, self.m)]
        var = [self.up(rng.standard_normal(max(self.n, 1))), self.up(rng.uniform(1, 2, max(self.m, 1))), self.up(rng.uniform(1, 2, max(self.m, 1)))]
        self._refusable(self.system.solve_dev, [p(t) for t in lhs], [p(t) for t in rhs], 0.5, 1.0, [p(t) for t in var], 1.0, 1.0, True)
        return True                                              # (accepted; how well K's scaled values condition is not the subject)

    def observe_qb(self):
        """(q, None, b): rx = -q and rz = -b at x = s = z = 0, tau = 1; -q is not readable (see the constant-RHS test)"""
        p = lambda t: t.data_ptr()
        rx, rxi, Px, rz, rzi = self.out
        self.system.residuals_dev(p(self.zx), p(self.zs), p(self.zz), 1.0, p(rx), p(rz), p(rxi), p(rzi), p(Px))
        return -rx[:self.n].cpu().numpy(), None, -rz[:self.m].cpu().numpy()

    def data_norms(self):
        return self.system.data_norms()


def observe_without_negq(dev, model):
    """du.check compares (q, -q, b); the device's -q is None: take the model's there"""
    q, _, b = Device.observe_qb(dev)
    return q, model.negq.copy(), b


MODERATE = dict(lo=0.5, hi=2.0)       # scalings under which the cases' K stays fit to factorise


def pair(case, scaled=True, seed=77, init=True, **span):
    rng = np.random.default_rng(78)
    q, b = rng.standard_normal(case.n), rng.standard_normal(case.m)
    dev = Device(case, q, b, init=init)
    K = dev.ks.KKT()
    model = du.model_of_case(case, K, dev.ks.maps())
    dev.observe_qb = lambda: observe_without_negq(dev, model)
    if init:
        model.init(q, b)
    if scaled:
        du.both(dev, model, "set_equilibration", *du.scalings(case.n, case.m, seed, **span))
    return dev, model


# ------------------------------------------------------------------------------------------------ the sequences
@pytest.mark.parametrize("name", ["segments", "block_edge[246,10]"])
def test_every_sequence(name):
    """d, e in [0.5, 2], c = 0.37: every sequence, the one that factorises and solves included"""
    case = kv.SMALL_CASES[name]()
    dev, model = pair(case, **MODERATE)
    assert model.c != 1.0 and model.d.min() == 0.5 and model.e.max() == 2.0
    du.run_all(dev, model, case)
    assert dev.ks.fallbacks == (0, 0)


@pytest.mark.parametrize("name", ["segments", "block_edge[246,10]"])
def test_value_sequences_with_scalings_over_eight_decades(name):
    """d, e from 1e-4 to 1e4, c = 0.37: every sequence that only compares values (c D P D then spans sixteen decades,
    which is more than a factorisation should be asked to take)"""
    case = kv.SMALL_CASES[name]()
    dev, model = pair(case)
    assert model.d.min() == 1e-4 and model.d.max() == 1e4 and model.e.min() == 1e-4 and model.e.max() == 1e4 and model.c != 1.0
    du.run_all(dev, model, case, factorise=False)


def test_every_sequence_with_scalings_never_set_and_cleared():
    case = kv.SMALL_CASES["segments"]()
    dev, model = pair(case, scaled=False)                     # never set: ones
    du.run_all(dev, model, case)
    dev, model = pair(case, scaled=True, **MODERATE)
    du.both(dev, model, "set_equilibration", None, None)     # set, then cleared
    assert model.c == 1.0 and (model.d == 1.0).all()
    du.run_all(dev, model, case, seed=5000)
    v = du.new_values(model.length("P"), 1)
    du.both(dev, model, "update_data", "P", v)
    assert np.array_equal(dev.ks.KKT().data[model.maps["P"]], v), "with scalings of one the values go in as they are"


def stacked(case, copies=2):
    return kv.Case("stack", sp.block_diag([case.P] * copies, format="csc"), sp.block_diag([case.A] * copies, format="csc"),
                   list(case.cones) * copies, case.seed)


def test_every_sequence_on_a_partitioned_handle():
    base = kv.SMALL_CASES["segments"]()
    case = stacked(base)
    dev, model = pair(case, **MODERATE)
    dev.system.set_problems([(base.n, base.m)] * 2)
    du.run_all(dev, model, case)


# ------------------------------------------------------------------------------------------------ lengths
def case_of_length(L):
    """n = m = nnz(A) = L, nnz(triu P) = 2 L - 1 (L = 1: 1)"""
    from cuclarabel_amd.cones import NonnegativeConeT
    rng = np.random.default_rng(600 + L)
    return kv.Case(f"len{L}", kv._tridiag_P(L, rng), kv._one_or_two_per_row(L, L, rng, None), [NonnegativeConeT(L)], 600 + L)


@pytest.mark.parametrize("L", [1, 255, 256, 257])
def test_vector_lengths_and_k_on_the_workgroup_edges(L):
    case = case_of_length(L)
    dev, model = pair(case, seed=L)
    assert (model.length("A"), model.length("q"), model.length("b")) == (L, L, L)
    du.check(dev, model, f"len{L} create")
    for which in ("A", "q", "b", "P"):
        du.both(dev, model, "update_data", which, du.new_values(model.length(which), L))
        du.check(dev, model, f"len{L} vector {which}")
        idx = np.random.default_rng(L).permutation(model.length(which))[:L]      # k = L positions
        du.both(dev, model, "update_data", which, du.new_values(L, L + 1), idx)
        du.check(dev, model, f"len{L} indexed {which}, k = {L}")
    assert dev.data_norms() == model.data_norms()


def test_one_length_past_the_grid_cap():
    """nnz(A) = 1 048 580 > 4096 x 256: the grid-stride loop's second trip in the vector form and in an indexed update of
    4096 x 256 + 1 entries; n = m = 209 716 for q and b.  The image is probed with two random columns (the bounded probe of
    tests/kvalue_reference.py), every new value at least a factor 4 off the one it replaces."""
    case = kv.case_banded_big()
    dev, model = pair(case, scaled=False)
    du.both(dev, model, "set_equilibration", *du.scalings(case.n, case.m, 9, lo=1.0, hi=2.0))     # (e d in [1, 4]: see the factors below)
    nA, cap = model.length("A"), du.UPDATE_GRID_CAP * du.UPDATE_BLOCK
    assert nA > cap
    du.check(dev, model, "big create")                                 # the image is current from here
    v = 16.0 * case.A.data
    du.both(dev, model, "update_data", "A", v)
    kv.assert_changed(case.A.data, model.Aval, "big vector A")
    du.check(dev, model, "big vector A", seed=1)
    idx = np.random.default_rng(3).permutation(nA)[:cap + 1]
    old = model.Aval[idx].copy()
    du.both(dev, model, "update_data", "A", case.A.data[idx] / 16.0, idx)
    kv.assert_changed(old, model.Aval[idx], "big indexed A")
    du.check(dev, model, "big indexed A", seed=2)
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 4))
    du.both(dev, model, "update_data", "b", du.new_values(case.m, 5))
    du.check(dev, model, "big q, b", seed=3)
    assert dev.data_norms() == model.data_norms()


# ------------------------------------------------------------------------------------------------ q, b, the norms
def test_negated_q_reaches_the_constant_rhs_solves():
    """-q is read by the constant-RHS solve and the initial point only: after update_data_q / _b the initial point equals,
    bit for bit, that of a second handle which got the scaled vectors through hipkkt_kkt_system_init."""
    case = kv.SMALL_CASES["segments"]()
    dev, model = pair(case, **MODERATE)
    du.both(dev, model, "update_data", "q", du.new_values(case.n, 31))
    du.both(dev, model, "update_data", "b", du.new_values(2, 32), np.array([case.m - 1, 0]))
    du.check(dev, model, "q, b")
    twin = Device(case, model.q, model.b)
    pts = []
    for w in (dev, twin):
        w.system_update(*case.hs(0))                            # (factorises; its constant-RHS solve reads -q and b)
        w.system.staging = "torch"
        ok, x, s, z = w.system.solve_initial_point()
        assert ok
        pts.append((x, s, z))
    for a, b_ in zip(*pts):
        assert a.tobytes() == b_.tobytes()
    assert np.abs(pts[0][0]).max() > 0


def test_data_norms_are_exact_also_with_an_empty_b_and_a_nan():
    from cuclarabel_amd.cones import NonnegativeConeT
    rng = np.random.default_rng(41)
    n = 300
    case = kv.Case("m0", kv._tridiag_P(n, rng), sp.csc_matrix((0, n)), [], 41)
    dev, model = pair(case)
    assert model.m == 0
    assert dev.data_norms() == model.data_norms() and model.data_norms()[1] == 0.0
    du.both(dev, model, "update_data", "q", du.new_values(n, 42))
    assert dev.data_norms() == model.data_norms()
    du.both(dev, model, "update_data", "q", np.array([-1e300]), np.array([n - 1]))       # the maximum in the last lane's entry
    assert dev.data_norms() == model.data_norms() and model.data_norms()[0] > 1e290
    du.both(dev, model, "update_data", "q", np.array([np.nan]), np.array([256]))
    assert np.isnan(dev.data_norms()[0])
    case = kv.Case("nn", kv._tridiag_P(8, rng), kv._one_or_two_per_row(40, 8, rng), [NonnegativeConeT(40)], 43)
    dev, model = pair(case)
    du.both(dev, model, "update_data", "b", np.array([np.inf]), np.array([39]))
    assert dev.data_norms() == model.data_norms() and dev.data_norms()[1] == np.inf


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_handle_as_it_was():
    case = kv.SMALL_CASES["segments"]()
    dev, model = pair(case, **MODERATE)
    du.check(dev, model, "create")
    nP, nA = model.length("P"), model.length("A")
    ones = lambda k: np.ones(k)
    for which, length in (("P", nP), ("A", nA), ("q", case.n), ("b", case.m)):
        for idx, pos in (([0, length], 1), ([-1, 0], 0), ([0, 1, 0], 2), ([1, 1, 0], 1), ([0, length - 1, 1, length - 1], 3)):
            du.expect_refused(dev, model, f"{which} {idx}",
                              lambda w, which=which, idx=idx: w.update_data(which, ones(len(idx)), np.array(idx)), pos=pos)
        du.expect_refused(dev, model, f"{which} wrong k", lambda w, which=which, length=length: w.update_data(which, ones(length + 1)))
        du.both(dev, model, "update_data", which, np.zeros(0))                        # k = 0: a no-op
        du.both(dev, model, "update_data", which, np.zeros(0), np.zeros(0, np.int64))
    du.check(dev, model, "after the no-ops")
    assert not model.const_stale and not model.factor_stale
    # a bad c, one pointer missing
    from cuclarabel_amd import _lib
    L, h = _lib.lib(), dev.ks._h
    d, e = _lib.f64(model.d), _lib.f64(model.e)
    for args in ((_lib.ptr(d), _lib.ptr(e), 0.0), (_lib.ptr(d), _lib.ptr(e), -1.0), (_lib.ptr(d), _lib.ptr(e), float("inf")),
                 (_lib.ptr(d), _lib.ptr(e), float("nan")), (_lib.ptr(d), None, 1.0), (None, _lib.ptr(e), 1.0)):
        assert L.hipkkt_kkt_system_set_equilibration(h, *args) == -1
    du.both(dev, model, "update_data", "P", du.values_like(case.P.data, 50))          # ... the scalings are still the old ones
    du.check(dev, model, "after the refused scalings")
    # stale reads: the factorisation after a P update, (x2, z2) after a q update
    from cuclarabel_amd._lib import HipKKTError
    dev.system_update(*case.hs(0))
    model.system_update(*case.hs(0))
    assert dev.solve()
    du.both(dev, model, "update_data", "b", du.new_values(1, 51), np.array([0]))
    du.expect_refused(dev, model, "solve after update_data_b", lambda w: w.solve())
    assert dev.system.solve_constant_rhs()                                            # (the factorisation is current: allowed)
    model.const_stale = False
    assert dev.solve()
    du.both(dev, model, "update_data", "A", du.new_values(1, 52), np.array([nA - 1]))
    du.expect_refused(dev, model, "solve after update_data_A", lambda w: w.solve())
    with pytest.raises(HipKKTError, match="stale"):
        dev.system.solve_constant_rhs()
    with pytest.raises(HipKKTError, match="stale"):
        dev.system.solve_initial_point_dev(dev.zx.data_ptr(), dev.zs.data_ptr(), dev.zz.data_ptr())
    du.check(dev, model, "after the refused solves")
    # deferred status
    dev.ks.set_deferred_status(True)
    model.deferred = True
    try:
        for which in "PAqb":
            for w in (dev, model):
                with pytest.raises(du.Refused):
                    w.update_data(which, ones(model.length(which)))
    finally:
        dev.ks.set_deferred_status(False)
        model.deferred = False
    du.check(dev, model, "after the deferred refusals")         # (level C reads nothing back in that mode: probed after it)
    du.both(dev, model, "system_update", *case.hs(1))
    assert dev.solve()
    du.check(dev, model, "at the end")


def test_q_and_b_need_init_and_P_and_A_do_not():
    case = kv.SMALL_CASES["segments"]()
    dev, model = pair(case, init=False)
    for which in "qb":
        with pytest.raises(du.Refused):
            dev.update_data(which, np.ones(model.length(which)))
        with pytest.raises(du.Refused):
            model.update_data(which, np.ones(model.length(which)))
    du.both(dev, model, "update_data", "P", du.new_values(model.length("P"), 60))
    du.both(dev, model, "update_data", "A", du.new_values(2, 61), np.array([3, 0]))
    kv.assert_values(dev.ks, model, "before init")
    kv.assert_image(dev.ks, model, "before init")
