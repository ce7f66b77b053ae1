"""hipkkt_kkt_system_residuals / _combined_rhs / _add_step (csrc/iterate_kernels.hip) against the exact reference and the
order-free bounds of tests/iterate_reference.py: one case per edge of the kernel, each at the smallest size that reaches
it -- row lengths around the eight lanes per row, m = 0, n = m = 1, a second trip of the grid-stride loop, long walked
prefixes around kLongRow, cones whose Hs blocks and expansion columns lie behind the A prefix, fresh values after
hipkkt_kkt_update_P / _A, the equilibration vectors, the norms' range, refusals.  Every call is made twice and must repeat
bit for bit in all five vectors and twelve scalars.  Worst error / bound per quantity is printed under -s."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd.cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT,
                                  GenPowerConeT)
from tests import iterate_reference as ir

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nhipkkt_kkt_system_residuals, worst error / bound:")
    for k in sorted(WORST):
        print(f"  {k:16s} {WORST[k][0]:.3g}  ({WORST[k][1]})")
    _DEVS.clear()                 # (the shared handles go before the interpreter does)
    _ELEM.clear()


def _within(ratios, where):
    for k, v in ratios.items():
        if k not in WORST or v > WORST[k][0]:
            WORST[k] = (v, where)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{where}: error / bound > 1 for {bad}"


class Dev:
    """a level-C handle over (P, A, cones) with system.init(q, b) and nothing else"""

    def __init__(self, P, A, cones, q, b):
        import torch
        from cuclarabel_amd import _lib
        from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
        assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
        self.torch = torch
        self.n, self.m = P.shape[0], A.shape[0]
        self.ks = HipKKTSolver(P, A, cones)
        self.system = HipKKTSystem(self.ks)
        self.system.init(q, b)

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        t = self.torch.zeros(max(a.size, 1), dtype=self.torch.float64, device="cuda")
        t[:a.size] = self.torch.from_numpy(a)
        self.torch.cuda.synchronize()
        return t

    def fill(self, k, v=float("nan")):
        t = self.torch.full((max(k, 1),), v, dtype=self.torch.float64, device="cuda")
        self.torch.cuda.synchronize()
        return t

    def down(self, t, k):
        self.ks.synchronize()
        return t.cpu().numpy()[:k].copy()

    def residuals(self, x, s, z, tau, equil=None):
        """-> (dict of the five vectors, array of 12); called twice on fresh NaN-filled outputs: identical bits"""
        n, m = self.n, self.m
        tx, ts, tz = self.up(x), self.up(s), self.up(z)
        eq = None if equil is None else [self.up(v) for v in equil]
        runs = []
        for _ in range(2):
            o = dict(rx=self.fill(n), rz=self.fill(m), rx_inf=self.fill(n), rz_inf=self.fill(m), Px=self.fill(n))
            scal = self.system.residuals_dev(tx.data_ptr(), ts.data_ptr(), tz.data_ptr(), tau, o["rx"].data_ptr(),
                                             o["rz"].data_ptr(), o["rx_inf"].data_ptr(), o["rz_inf"].data_ptr(),
                                             o["Px"].data_ptr(), None if eq is None else [t.data_ptr() for t in eq])
            runs.append(({k: self.down(t, n if k in ("rx", "rx_inf", "Px") else m) for k, t in o.items()}, scal.copy()))
        for k in ir.VECTORS:
            assert runs[0][0][k].tobytes() == runs[1][0][k].tobytes(), f"{k}: the same call on the same data gave other bits"
        assert runs[0][1].tobytes() == runs[1][1].tobytes(), "scalars: the same call on the same data gave other bits"
        assert self.down(tx, n).tobytes() == np.ascontiguousarray(x, dtype=np.float64).tobytes(), "an input was modified"
        return runs[0]


_DEVS = {}


def _dev(name):
    if name not in _DEVS:
        pb = ir.problem(name)
        _DEVS[name] = Dev(pb.P, pb.A, pb.cones, pb.q, pb.b)
    return _DEVS[name]


def _check(pb, vec, scal, where, equil=None, exact=None, bounds=None, data=None):
    data = data or pb.data()
    r = ir.vector_ratios(pb, data, vec, exact, bounds)
    r.update(ir.scalar_ratios(data, vec, scal, equil))
    assert set(r) == set(ir.VECTORS) | set(ir.SCALARS)
    _within(r, where)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ir.BUILDERS))
def test_vectors_and_scalars_within_bound(name):
    """edges: P rows, A rows and A columns of 0, 1, 7, 8, 9, 64, 65 entries, a variable in no constraint, an empty row of
    A; lp: P = 0; unconstrained: m = 0; n1m1; wrap: n = m = 65 537 + 31, the grid-stride loop's further trips;
    dense_row_L / dense_col_L: a walked prefix of kLongRow - 1, kLongRow, kLongRow + 1, 3 kLongChunk + 1 entries in a z row
    and in an x row.  Without and with the four equilibration vectors."""
    pb, dev = ir.problem(name), _dev(name)
    vec, scal = dev.residuals(pb.x, pb.s, pb.z, pb.tau)
    _check(pb, vec, scal, name, None, pb.exact, pb.bounds)
    eq = ir.equil_vectors(pb)
    vec2, scal2 = dev.residuals(pb.x, pb.s, pb.z, pb.tau, eq)
    for k in ir.VECTORS:
        assert vec2[k].tobytes() == vec[k].tobytes(), "the equilibration vectors must not change a vector"
    assert scal2[:4].tobytes() == scal[:4].tobytes()
    _check(pb, vec2, scal2, name + " equilibrated", eq, pb.exact, pb.bounds)


def _interior(cones, rng):
    """a strictly interior (s, z) for zero / nonnegative / second-order / PSD / exponential / generalized power cones"""
    from cuclarabel_amd.problems import interior_point
    out = []
    for c in cones:
        if isinstance(c, ExponentialConeT):
            s, z = np.array([-1.0, 1.0, 1.0]), np.array([-1.0, 1.0, 1.0])       # y e^(x/y) = 1/e < 1; -u e^(v/u) = 1/e < e w
        elif isinstance(c, GenPowerConeT):
            d1 = c.numel - 2
            s = z = np.r_[np.ones(d1), 0.1, 0.1]                                   # prod x^a = 1 > 0.15; prod (u/a)^a > 1
        else:
            s, z = interior_point([c], rng), interior_point([c], rng)
        out.append((s, z))
    return np.concatenate([p[0] for p in out]), np.concatenate([p[1] for p in out])


def test_nothing_behind_the_A_prefix_is_read():
    """SOC(65) (sparse expansion columns), PSD(8) (dense Hs block), an exponential and a generalized power cone: the
    residuals work before the first update at all, and after an update from an interior (s, z) -- Hs blocks and expansion
    columns filled -- they are those of the same P, A bit for bit."""
    from cuclarabel_amd import ipm
    rng = np.random.default_rng(61)
    cones = [NonnegativeConeT(3), SecondOrderConeT(65), PSDTriangleConeT(8), ExponentialConeT(), GenPowerConeT([0.4, 0.6], 2),
             ZeroConeT(2)]
    m = sum(c.numel for c in cones)
    n = 30
    A = sp.random(m, n, density=0.3, random_state=np.random.RandomState(5), format="csc")
    P = sp.diags([rng.uniform(1.0, 2.0, n), rng.uniform(-0.2, 0.2, n - 1)], [0, 1], format="csc")
    pb = ir.Problem("hs", P, A, cones, 62)
    dev = Dev(pb.P, pb.A, cones, pb.q, pb.b)
    vec0, scal0 = dev.residuals(pb.x, pb.s, pb.z, pb.tau)
    _check(pb, vec0, scal0, "cones behind A, before any update")
    s, z = _interior(cones, rng)
    dev.ks.set_nonsymmetric_scaling(ipm.DUAL, 1.0)
    assert dev.ks.kktsolver_update_from_sz(s, z)
    K = dev.ks.KKT()
    assert np.count_nonzero(K.data) > pb.P.nnz + pb.A.nnz + m, "the update filled the Hs blocks and expansion columns"
    vec1, scal1 = dev.residuals(pb.x, pb.s, pb.z, pb.tau)
    for k in ir.VECTORS:
        assert vec1[k].tobytes() == vec0[k].tobytes(), k
    assert scal1.tobytes() == scal0.tobytes()


def _nn_problem(seed):
    rng = np.random.default_rng(seed)
    n, m = 25, 40
    A = sp.random(m, n, density=0.25, random_state=np.random.RandomState(seed), format="csc")
    P = sp.diags([rng.uniform(1.0, 2.0, n), rng.uniform(-0.2, 0.2, n - 1)], [0, 1], format="csc")
    return ir.Problem("fresh", P, A, [ZeroConeT(4), NonnegativeConeT(m - 4)], seed + 1)


@pytest.mark.parametrize("lazy", [False, True])
def test_fresh_values_after_update_P_and_update_A(lazy):
    """after hipkkt_kkt_update_A and _update_P with no solve in between the residuals are those of the new matrices --
    also in lazy mode with an update pending"""
    pb = _nn_problem(71)
    dev = Dev(pb.P, pb.A, pb.cones, pb.q, pb.b)
    vec, scal = dev.residuals(pb.x, pb.s, pb.z, pb.tau)               # (the image's values are now current: not dirty)
    _check(pb, vec, scal, "before the data update")
    rng = np.random.default_rng(72)
    P2, A2 = pb.P.copy(), pb.A.copy()
    P2.data = P2.data * rng.uniform(0.5, 1.5, P2.nnz)
    A2.data = A2.data * rng.uniform(0.5, 1.5, A2.nnz)
    if lazy:
        dev.system.set_lazy(True)
        sz = dev.up(np.abs(pb.s) + 0.5), dev.up(np.abs(pb.z) + 0.5)
        assert dev.system.update_dev(sz[0].data_ptr(), sz[1].data_ptr())       # enqueued only
    dev.ks.kktsolver_update_A(A2)
    dev.ks.kktsolver_update_P(P2)
    new = ir.Problem("fresh2", P2, A2, pb.cones, 71 + 1)
    assert new.x.tobytes() == pb.x.tobytes()
    vec2, scal2 = dev.residuals(pb.x, pb.s, pb.z, pb.tau)
    _check(new, vec2, scal2, "after update_A and update_P" + (" (lazy, update pending)" if lazy else ""))
    stale = ir.vector_ratios(new, new.data(), vec)
    assert min(stale[k] for k in ("Px", "rx_inf", "rz_inf")) > 1.0, "the old matrices' residuals would not have passed"
    if lazy:
        dev.system.set_lazy(False)


def test_equilibration_vectors_all_or_none_and_deferred_status():
    """a mixed set of equilibration vectors returns -1 and writes nothing (sentinel buffers); so does a deferred-status
    handle, which works again afterwards"""
    import torch
    from cuclarabel_amd import _lib
    pb = _nn_problem(81)
    dev = Dev(pb.P, pb.A, pb.cones, pb.q, pb.b)
    L, h = _lib.lib(), dev.ks._h
    n, m = pb.n, pb.m
    tx, ts, tz = dev.up(pb.x), dev.up(pb.s), dev.up(pb.z)
    eq = [dev.up(v) for v in ir.equil_vectors(pb)]
    P = lambda t: None if t is None else t.data_ptr()

    def refused(eqs, others=True):
        o = [dev.fill(k, 7.0) for k in (n, m, n, m, n)]
        out = np.full(12, 7.0)
        calls = [lambda: L.hipkkt_kkt_system_residuals(h, P(tx), P(ts), P(tz), 0.7, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]),
                                                        P(eqs[0]), P(eqs[1]), P(eqs[2]), P(eqs[3]), _lib.ptr(out))]
        if others:
            calls += [lambda: L.hipkkt_kkt_system_combined_rhs(h, P(o[0]), P(o[1]), P(tx), P(ts), 0.5),
                      lambda: L.hipkkt_kkt_system_add_step(h, P(o[0]), P(o[1]), P(o[3]), P(tx), P(ts), P(tz), 0.5)]
        for call in calls:
            assert call() == -1, L.hipkkt_last_error()                 # HIPKKT_ERR_ARG
            assert L.hipkkt_last_error()
        dev.ks.synchronize()
        torch.cuda.synchronize()
        assert all(np.all(t.cpu().numpy() == 7.0) for t in o) and np.all(out == 7.0), "a refused call wrote something"

    for missing in range(4):
        refused([None if i == missing else eq[i] for i in range(4)], others=False)
    refused([eq[0], None, None, None], others=False)
    # a step that aliases the vector it is added to, and s aliasing z
    v = [dev.fill(k, 7.0) for k in (n, m, m)]
    for args in ((P(v[0]), P(v[1]), P(v[2]), P(v[0]), P(ts), P(tz)), (P(v[0]), P(v[1]), P(v[2]), P(tx), P(v[2]), P(tz)),
                 (P(v[0]), P(v[1]), P(v[1]), P(tx), P(ts), P(tz))):
        assert L.hipkkt_kkt_system_add_step(h, *args, 0.5) == -1 and L.hipkkt_last_error()
    dev.ks.synchronize()
    assert all(np.all(t.cpu().numpy() == 7.0) for t in v)
    dev.ks.set_deferred_status(True)
    refused(eq)
    refused([None] * 4)
    dev.ks.set_deferred_status(False)
    assert dev.ks.deferred_status() in (0, 1, 2)
    vec, scal = dev.residuals(pb.x, pb.s, pb.z, pb.tau, ir.equil_vectors(pb))
    _check(pb, vec, scal, "after the refusals", ir.equil_vectors(pb))


def test_norm_range_zero_and_nan():
    """entries of 1e200 and of 1e-200 in x and in s: the norms are finite, nonzero and within bound; a zero iterate gives
    exactly 0 everywhere; one NaN in z makes every scalar that depends on z non-finite and no other"""
    pb = _nn_problem(91)
    dev = Dev(pb.P, pb.A, pb.cones, pb.q, pb.b)
    eq = ir.equil_vectors(pb)
    for scale, where in ((1e200, "1e200"), (1e-200, "1e-200")):
        for equil in (None, eq):
            x, s = pb.x * scale, pb.s * scale
            z = pb.z * (scale if scale < 1 else 1.0)
            data = dict(pb.data(), x=x, s=s, z=z)
            vec, scal = dev.residuals(x, s, z, pb.tau, equil)
            norms = scal[4:]
            assert np.isfinite(norms).all() and (norms > 0).all(), (where, norms)
            assert all(np.isfinite(v).all() for v in vec.values())
            _within(ir.scalar_ratios(data, vec, scal, equil, dots=False), f"range {where}" + (" equilibrated" if equil else ""))
    # entries of both magnitudes in one vector, and a few ordinary ones
    x, s = pb.x.copy(), pb.s.copy()
    x[::3] *= 1e200
    x[1::3] *= 1e-200
    s[::2] *= 1e-200
    s[1] *= 1e200
    vec, scal = dev.residuals(x, s, pb.z, pb.tau, eq)
    assert np.isfinite(scal[4:]).all() and (scal[4:] > 0).all()
    _within(ir.scalar_ratios(dict(pb.data(), x=x, s=s), vec, scal, eq, dots=False), "range mixed")
    # zero
    vec, scal = dev.residuals(np.zeros(pb.n), np.zeros(pb.m), np.zeros(pb.m), 0.0, eq)
    assert np.all(scal == 0.0) and all(np.all(v == 0.0) for v in vec.values())
    # NaN
    z = pb.z.copy()
    k = int(np.flatnonzero(pb.parts.kz > 0)[0])
    z[k] = float("nan")
    vec, scal = dev.residuals(pb.x, pb.s, z, pb.tau, eq)
    S = dict(zip(ir.SCALARS, scal))
    for name in ("bz", "sz", "n_ez", "n_dinv_rx_inf", "n_dinv_rx"):
        assert not math.isfinite(S[name]), name
    for name in ("qx", "xPx", "n_dx", "n_einv_s", "n_dinv_Px", "n_einv_rz_inf", "n_einv_rz"):
        assert math.isfinite(S[name]), name


# ---------------------------------------------------------------------------------------------------------------------
ELEM_CAP = ir.ELEM_GRID_CAP * 256
_ELEM = {}


def _elem_dev(n, m):
    if (n, m) not in _ELEM:
        P = sp.identity(n, format="csc")
        A = sp.csc_matrix((np.ones(min(n, m)), (np.arange(min(n, m)), np.arange(min(n, m)))), shape=(m, n))
        _ELEM[(n, m)] = Dev(P, A, [NonnegativeConeT(m)] if m else [], np.zeros(n), np.zeros(m))
    return _ELEM[(n, m)]


ELEM_SHAPES = [(1, 0), (255, 0), (256, 0), (257, 0), (ELEM_CAP + 1, 0), (100, 57), (1, 1)]


@pytest.mark.parametrize("n,m", ELEM_SHAPES)
def test_combined_rhs_is_exact_and_may_alias(n, m):
    """rhs = fl((1 - sigma) r) exactly (the file is built without contraction): total lengths 1, 255, 256, 257 and one
    above the capped grid; x and z parts in one launch; outputs aliasing inputs"""
    dev = _elem_dev(n, m)
    rng = np.random.default_rng(n + 3 * m)
    rx, rz, sigma = rng.standard_normal(n), rng.standard_normal(m), 0.37
    want = ((1.0 - sigma) * rx, (1.0 - sigma) * rz)
    trx, trz, ox, oz = dev.up(rx), dev.up(rz), dev.fill(n), dev.fill(m)
    for _ in range(2):
        assert dev.system.combined_rhs_dev(ox.data_ptr(), oz.data_ptr(), trx.data_ptr(), trz.data_ptr(), sigma)
        assert dev.down(ox, n).tobytes() == want[0].tobytes() and dev.down(oz, m).tobytes() == want[1].tobytes()
    assert dev.down(trx, n).tobytes() == rx.tobytes() and dev.down(trz, m).tobytes() == rz.tobytes()
    assert dev.system.combined_rhs_dev(trx.data_ptr(), trz.data_ptr(), trx.data_ptr(), trz.data_ptr(), sigma)     # in place
    assert dev.down(trx, n).tobytes() == want[0].tobytes() and dev.down(trz, m).tobytes() == want[1].tobytes()


@pytest.mark.parametrize("n,m", ELEM_SHAPES)
def test_add_step_is_exact(n, m):
    """v = fl(v + fl(alpha d)) exactly for x, s and z in one launch"""
    dev = _elem_dev(n, m)
    rng = np.random.default_rng(7 * n + m)
    v = [rng.standard_normal(k) for k in (n, m, m)]
    d = [rng.standard_normal(k) for k in (n, m, m)]
    alpha = 0.8125 + 2.0 ** -30
    want = [a + alpha * b for a, b in zip(v, d)]
    tv, td = [dev.up(a) for a in v], [dev.up(a) for a in d]
    assert dev.system.add_step_dev(tv[0].data_ptr(), tv[1].data_ptr(), tv[2].data_ptr(), td[0].data_ptr(), td[1].data_ptr(),
                                   td[2].data_ptr(), alpha)
    for t, w, b, src in zip(tv, want, td, d):
        assert dev.down(t, w.size).tobytes() == w.tobytes()
        assert dev.down(b, w.size).tobytes() == src.tobytes(), "a step was modified"
